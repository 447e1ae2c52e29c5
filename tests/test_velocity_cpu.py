"""CPU suite of the body-velocity (DVL) update (include/fbus_ekf.h, fbus_ekf_correct_velocity*; added under FBUS_ABI_VERSION 8 without a
bump): the six symbols and their null-handle checks, the unit that builds the kernel, the Python and C++ layers, tests/velocity_ref.py -- the
fp64 restatement the GPU suite holds the kernel to -- against central differences of its own h and against the identities between the
joint and the sequential form of a three-row update, and the sharding of synth.velocity."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest

import ekf_oracle_np as E
import velocity_ref as V
from fbus_ekf import capi, synth
from util import cov_rel_err_blockwise

NEW = ["fbus_ekf_set_velocity_sensor", "fbus_ekf_correct_velocity", "fbus_ekf_correct_velocity_dev", "fbus_ekf_correct_velocity_async",
       "fbus_ekf_correct_velocity_nis", "fbus_ekf_correct_velocity_nis_dev"]
MOUNT = V.tilted_mount()
LEVER = np.array([0.21, -0.08, 0.12])
GYRO = np.array([0.05, -0.11, 0.07])
VAR = np.array([1e-4, 4e-4, 2.5e-5])


def test_the_six_symbols_are_declared_exported_and_refuse_a_null_handle():
    declared = capi.declared_symbols()
    lib = capi.load_library()
    for n in NEW:
        assert n in declared, n
        assert hasattr(lib, n), n
    assert capi.ABI_VERSION == 8 and lib.fbus_ekf_abi_version() == 8
    mt = (C.c_double * 9)(1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)
    z = (C.c_float * 12)()
    var = (C.c_double * 12)(*([1.0] * 12))
    assert lib.fbus_ekf_set_velocity_sensor(None, mt, None) == 1
    assert lib.fbus_ekf_set_velocity_sensor(None, None, None) == 1
    for fn in ("fbus_ekf_correct_velocity", "fbus_ekf_correct_velocity_dev", "fbus_ekf_correct_velocity_async"):
        assert getattr(lib, fn)(None, z, z, var, 0, None) == 1
        assert getattr(lib, fn)(None, None, None, None, 2, None) == 1
    for fn in ("fbus_ekf_correct_velocity_nis", "fbus_ekf_correct_velocity_nis_dev"):
        assert getattr(lib, fn)(None, z, None, var, 1, None, None, None) == 1


def test_the_kernel_builds_in_its_family_unit(repo_root):
    spec = importlib.util.spec_from_file_location("fbus_build_velocity", os.path.join(repo_root, "fbus-ekf_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert any(h.endswith("ekf_velocity.hpp") for h in b.HEADERS)            # a change of the kernel rebuilds the library
    assert any(h.endswith("ekf_sensor.hpp") for h in b.HEADERS)            # ... and so does one of the steps it shares
    csrc = os.path.join(repo_root, "fbus-ekf_amd", "csrc")
    units = [u for u in b.units() if u[0].endswith("_sensor")]
    assert sorted(u[0] for u in units) == ["f32_15_sensor", "f32_18_sensor", "f64_15_sensor", "f64_18_sensor"]
    assert {u[1] for u in units} == {os.path.join(csrc, "small_tu.hip")}
    # the family's branch of the unit source includes the header (over the steps the three sensor updates share): that unit instantiates the kernel
    code = b.FAMILIES["sensor"][0]
    tu = open(os.path.join(csrc, "small_tu.hip")).read()
    assert re.search(rf'#elif FBUS_TU_FAMILY == {code}\n(?:#include "ekf_\w+\.hpp"\n)*?#include "ekf_velocity.hpp"\n', tu)
    assert all(f"-DFBUS_TU_FAMILY={code}" in u[2] for u in units)
    assert '#include "ekf_sensor.hpp"' in open(os.path.join(csrc, "ekf_velocity.hpp")).read()
    main = open(os.path.join(csrc, "fbus_ekf.hip")).read()
    assert '#include "ekf_velocity.hpp"' not in main                                  # ... and the host unit does not


def test_the_python_and_cxx_layers_carry_the_methods(repo_root):
    from fbus_ekf import BatchedFilter
    for m in ("set_velocity_sensor", "correct_velocity", "correct_velocity_nis", "correct_velocity_async"):
        assert callable(getattr(BatchedFilter, m))
    hdr = open(os.path.join(repo_root, "include", "fbus", "batched_filter.hpp")).read()
    for m in ("set_velocity_sensor", "correct_velocity", "correct_velocity_dev", "correct_velocity_async", "correct_velocity_nis",
              "correct_velocity_nis_dev"):
        assert f"void {m}(" in hdr, m


# ---- velocity_ref against itself ------------------------------------------------------------------------------------------------------------

def _state(n, seed):
    """a state with a NON-orthonormal carried rotation (what a run of predicts leaves), a velocity of ~0.3 m/s and a dense covariance"""
    rng = np.random.default_rng(seed)
    s = E.State(n)
    s.p, s.v = rng.uniform(-1, 1, 3), rng.normal(0, 0.3, 3)
    q = rng.normal(size=4)
    s.q = q / np.linalg.norm(q)
    s.R = E.q2R(s.q) + rng.normal(0, 1e-3, (3, 3))
    s.ba, s.bg, s.g = rng.normal(0, 0.05, 3), rng.normal(0, 0.002, 3), np.array([9.8, 0.0, 0.0])
    A = np.eye(n) + rng.normal(0, 0.05, (n, n))
    d = np.sqrt(E.Params(E.CPP, n).P0().diagonal())
    s.P = d[:, None] * (A @ A.T) * d[None, :]
    s.P = (s.P + s.P.T) / 2
    return s


CASES = [(MOUNT, LEVER, GYRO), (None, LEVER, GYRO), (MOUNT, None, GYRO), (MOUNT, LEVER, None), (None, None, None)]


@pytest.mark.parametrize("n", [18, 15])
def test_H_is_the_derivative_of_h(n):
    """central differences of velocity_ref.h: v and bg additively, R <- R exp([d]x) -- the injection's convention q <- q (x) dq(dtheta)"""
    for seed in range(4):
        s = _state(n, seed)
        for mount, lever, gyro in CASES:
            Cm, lv = V.mount_of(mount), V.lever_of(lever)
            H = V.H_rows(s, n, Cm, lv, gyro)
            assert H.shape == (3, n)
            eps = 1e-6
            num = np.zeros((3, n))
            for i in range(3):
                d = np.zeros(3)
                d[i] = eps
                sp, sm = s.copy(), s.copy()
                sp.v, sm.v = s.v + d, s.v - d
                num[:, 3 + i] = (V.h(sp, Cm, lv, gyro) - V.h(sm, Cm, lv, gyro)) / (2 * eps)
                sp, sm = s.copy(), s.copy()
                K = E.skew(d)
                ex = np.eye(3) + np.sin(eps) / eps * K + (1 - np.cos(eps)) / eps ** 2 * (K @ K)       # exp([d]x), |d| = eps
                sp.R, sm.R = s.R @ ex, s.R @ ex.T
                num[:, 6 + i] = (V.h(sp, Cm, lv, gyro) - V.h(sm, Cm, lv, gyro)) / (2 * eps)
                sp, sm = s.copy(), s.copy()
                sp.bg, sm.bg = s.bg + d, s.bg - d
                num[:, 12 + i] = (V.h(sp, Cm, lv, gyro) - V.h(sm, Cm, lv, gyro)) / (2 * eps)
            err = np.abs(H - num).max()
            assert err <= 1e-7, err
            assert np.all(H[:, 0:3] == 0) and np.all(H[:, 9:12] == 0) and np.all(H[:, 15:] == 0)


def test_without_gyro_or_without_a_lever_the_bg_columns_are_exactly_zero():
    for n in (18, 15):
        s = _state(n, 3)
        for lever, gyro in ((LEVER, None), (None, GYRO), (np.zeros(3), GYRO), (None, None)):
            H = V.H_rows(s, n, MOUNT, V.lever_of(lever), gyro)
            assert np.all(H[:, 12:15] == 0.0)
            assert np.array_equal(H[:, 3:6], MOUNT @ s.R.T)
        # and then h does not see the gyro either
        assert np.array_equal(V.h(s, MOUNT, V.lever_of(None), GYRO), V.h(s, MOUNT, V.lever_of(LEVER), None))


@pytest.mark.parametrize("n", [18, 15])
def test_the_covariance_forms_are_one_matrix_and_the_sequential_rows_are_the_joint_solve(n):
    for seed in range(4):
        s = _state(n, 10 + seed)
        var = VAR * 10.0 ** (seed - 2)
        Cm = V.mount_of(MOUNT)
        H = V.H_rows(s, n, Cm, LEVER, GYRO)
        z = V.h(s, Cm, LEVER, GYRO) + np.array([0.01, -0.02, 0.005])
        res = z - V.h(s, Cm, LEVER, GYRO)
        lit, jos = s.copy(), s.copy()
        r1 = V.correct_velocity(lit, n, z, var, GYRO, MOUNT, LEVER)
        r2 = V.correct_velocity(jos, n, z, var, GYRO, MOUNT, LEVER, joseph=True)
        assert r1 == r2 and r1[0] and r1[2] == 3
        jn = V.joint(s.P, H, var)
        sq, dx, nis, lnd, ss = V.sequential(s.P, H, var, res)
        for a, b in ((lit.P, jn), (jos.P, jn), (jos.P, lit.P), (sq, jn), (sq, lit.P)):
            assert cov_rel_err_blockwise(a[None], b[None]) < 1e-12
        # nis, ln det S and the pivots of the sequential form are the joint solve's
        S = H @ s.P @ H.T + np.diag(var)
        assert abs(nis - res @ np.linalg.solve(S, res)) <= 1e-12 * nis and abs(nis - r1[1]) <= 1e-12 * nis
        assert abs(lnd - np.linalg.slogdet(S)[1]) <= 1e-12 * abs(lnd) and abs(lnd - r1[3]) <= 1e-12 * abs(lnd)
        assert np.abs(ss - np.diag(np.linalg.cholesky(S)) ** 2).max() <= 1e-12 * ss.max()
        assert np.abs(ss - V.pivots_of(S)).max() <= 1e-12 * ss.max()
        # dx of the sequential form is K res, and the state moved along it
        Kres = s.P @ H.T @ np.linalg.solve(S, res)
        assert np.abs(dx - Kres).max() <= 1e-12 * np.abs(Kres).max()
        assert np.abs(lit.v - s.v - Kres[3:6]).max() < 1e-15 and np.abs(lit.bg - s.bg - Kres[12:15]).max() < 1e-15
        # the joint identity: H P+ H' = R - R S^-1 R
        Rm = np.diag(var)
        for post in (lit.P, jos.P, jn, sq):
            assert np.abs(H @ post @ H.T - (Rm - Rm @ np.linalg.solve(S, Rm))).max() <= 1e-12 * np.abs(S).max()


def test_untouched_filters_the_pivots_and_the_gate():
    s = _state(18, 5)
    z0 = V.h(s, MOUNT, LEVER, GYRO)
    nan3, bad = np.array([0.0, np.nan, 0.0]), GYRO.copy()
    bad[2] = np.inf
    for z, var, gyro, skip in ((z0 + nan3, VAR, GYRO, False), (z0 + np.array([np.inf, 0, 0]), VAR, GYRO, False),
                               (z0, VAR * [1, 0, 1], GYRO, False), (z0, VAR * [1, 1, -1], GYRO, False), (z0, VAR + nan3, GYRO, False),
                               (z0, VAR * [np.inf, 1, 1], GYRO, False), (z0, VAR, GYRO + nan3, False), (z0, VAR, bad, False),
                               (z0, VAR, GYRO, True)):
        t = s.copy()
        assert V.correct_velocity(t, 18, z, var, gyro, MOUNT, LEVER, skip=skip)[:3] == (False, 0.0, 0)
        assert np.array_equal(t.P, s.P) and np.array_equal(t.v, s.v) and np.array_equal(t.q, s.q)
    # a non-finite gyro does not matter where no gyro is given
    assert V.usable(z0, VAR, None) and not V.usable(z0, VAR, GYRO + nan3)
    t = s.copy()
    ok, nis, dof, _ = V.correct_velocity(t, 18, z0 + 5.0, VAR, GYRO, MOUNT, LEVER, thr3=10.0)
    assert not ok and nis > 10.0 and dof == 3 and np.array_equal(t.P, s.P)
    t = s.copy()
    ok, nis, dof, _ = V.correct_velocity(t, 18, z0 + 0.001, VAR, GYRO, MOUNT, LEVER, thr3=10.0)
    assert ok and nis <= 10.0 and dof == 3 and not np.array_equal(t.P, s.P)
    # a covariance that is not positive on the rows: a pivot <= 0 is not applied, whatever the gate
    t = s.copy()
    t.P = -t.P * 1e3
    u = t.copy()
    ok, nis, dof, _ = V.correct_velocity(u, 18, z0, VAR, GYRO, MOUNT, LEVER)
    assert not ok and dof == 3 and np.array_equal(u.P, t.P)
    # a NaN record: nis is NaN, both comparisons are false
    t = s.copy()
    t.P = t.P * np.nan
    ok, nis, dof, _ = V.correct_velocity(t, 18, z0, VAR, GYRO, MOUNT, LEVER)
    assert not ok and np.isnan(nis) and dof == 3


# ---- synth.velocity ---------------------------------------------------------------------------------------------------------------------------

def test_two_shards_cut_inside_a_block_reproduce_the_unsharded_stream():
    B, cut = 2500, 1500                                   # the cut lies inside the second 1024-filter block
    nom, rot, _, _ = synth.initial_state(0, B, [1e-4] * 6, 18, with_cov=False)
    _, gyr = synth.imu_samples(0, B, 0, 1, nom)
    gyr = gyr[0]
    kw = dict(mount=MOUNT, lever=LEVER, noise=0.02)
    for step in (0, 3):
        whole = synth.velocity(0, B, step, nom, rot, gyr, **kw)
        a = synth.velocity(0, cut, step, nom[:cut], rot[:cut], gyr[:cut], **kw)
        b = synth.velocity(cut, B, step, nom[cut:], rot[cut:], gyr[cut:], **kw)
        assert whole.shape == (B, 3) and whole.dtype == np.float64
        assert np.array_equal(np.concatenate([a, b]), whole)
    assert not np.array_equal(synth.velocity(0, B, 0, nom, rot, gyr, **kw), synth.velocity(0, B, 1, nom, rot, gyr, **kw))
    # its stream is its own: not the depth stream's numbers
    assert not np.array_equal(synth.velocity(0, B, 0, nom * 0, rot, None, noise=1.0)[:, 0], synth.depth(0, B, 0, nom * 0, rot, noise=1.0))
    # the values are the model's: noise-free, z = C (R' v + (gyro - bg) x lever)
    z0 = synth.velocity(0, 64, 0, nom[:64], rot[:64], gyr[:64], mount=MOUNT, lever=LEVER, noise=0.0)
    ss = V.states_of((nom[:64], rot[:64], np.zeros((64, 18, 18)), np.zeros(64, np.int32)), 18)
    ref = np.array([V.h(ss[b], MOUNT, LEVER, gyr[b]) for b in range(64)])
    assert np.abs(z0 - ref).max() < 1e-15 * 4
    # rot_true = None: the rotation of the quaternion; no gyro, mount or lever: z = R' v
    assert np.abs(synth.velocity(0, 64, 0, nom[:64], None, gyr[:64], mount=MOUNT, lever=LEVER, noise=0.0) - z0).max() < 1e-12
    z1 = synth.velocity(0, 64, 0, nom[:64], rot[:64], noise=0.0)
    assert np.abs(z1 - np.einsum("bji,bj->bi", rot[:64].reshape(-1, 3, 3), nom[:64, 3:6])).max() < 1e-15
