"""CPU suite of the depth (pressure) sensor update (include/fbus_ekf.h, fbus_ekf_correct_depth*; added under FBUS_ABI_VERSION 8 without a
bump): the six symbols and their null-handle checks, the unit that builds the kernel, the Python and C++ layers, tests/depth_ref.py -- the
fp64 restatement the GPU suite holds the kernel to -- against central differences of its own h and against the identities of a scalar
update, and the sharding of synth.depth."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest

import depth_ref
import ekf_oracle_np as E
from fbus_ekf import capi, synth
from util import cov_rel_err_blockwise

NEW = ["fbus_ekf_set_depth_sensor", "fbus_ekf_correct_depth", "fbus_ekf_correct_depth_dev", "fbus_ekf_correct_depth_async",
       "fbus_ekf_correct_depth_nis", "fbus_ekf_correct_depth_nis_dev"]
AXIS = np.array([0.12, -0.2, 1.0])                   # tilted: every component of H_p and of R' axis is in play
LEVER = np.array([0.11, -0.07, 0.05])


def test_the_six_symbols_are_declared_exported_and_refuse_a_null_handle():
    declared = capi.declared_symbols()
    lib = capi.load_library()
    for n in NEW:
        assert n in declared, n
        assert hasattr(lib, n), n
    assert capi.ABI_VERSION == 8 and lib.fbus_ekf_abi_version() == 8
    ax = (C.c_double * 3)(0.0, 0.0, 1.0)
    z = (C.c_float * 4)()
    var = (C.c_double * 4)(1.0, 1.0, 1.0, 1.0)
    assert lib.fbus_ekf_set_depth_sensor(None, ax, 0.0, None) == 1
    assert lib.fbus_ekf_set_depth_sensor(None, None, 0.0, None) == 1
    for fn in ("fbus_ekf_correct_depth", "fbus_ekf_correct_depth_dev", "fbus_ekf_correct_depth_async"):
        assert getattr(lib, fn)(None, z, var, 0, None) == 1
        assert getattr(lib, fn)(None, None, None, 2, None) == 1
    for fn in ("fbus_ekf_correct_depth_nis", "fbus_ekf_correct_depth_nis_dev"):
        assert getattr(lib, fn)(None, z, var, 1, None, None, None) == 1


def test_the_kernel_builds_in_its_family_unit(repo_root):
    spec = importlib.util.spec_from_file_location("fbus_build_depth", os.path.join(repo_root, "fbus-ekf_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert any(h.endswith("ekf_depth.hpp") for h in b.HEADERS)            # a change of the kernel rebuilds the library
    assert any(h.endswith("ekf_sensor.hpp") for h in b.HEADERS)            # ... and so does one of the steps it shares
    csrc = os.path.join(repo_root, "fbus-ekf_amd", "csrc")
    units = [u for u in b.units() if u[0].endswith("_sensor")]
    assert sorted(u[0] for u in units) == ["f32_15_sensor", "f32_18_sensor", "f64_15_sensor", "f64_18_sensor"]
    assert {u[1] for u in units} == {os.path.join(csrc, "small_tu.hip")}
    # the family's branch of the unit source includes the header (over the steps the three sensor updates share): that unit instantiates the kernel
    code = b.FAMILIES["sensor"][0]
    tu = open(os.path.join(csrc, "small_tu.hip")).read()
    assert re.search(rf'#elif FBUS_TU_FAMILY == {code}\n(?:#include "ekf_\w+\.hpp"\n)*?#include "ekf_depth.hpp"\n', tu)
    assert all(f"-DFBUS_TU_FAMILY={code}" in u[2] for u in units)
    assert '#include "ekf_sensor.hpp"' in open(os.path.join(csrc, "ekf_depth.hpp")).read()
    main = open(os.path.join(csrc, "fbus_ekf.hip")).read()
    assert '#include "ekf_depth.hpp"' not in main                                  # ... and the host unit does not


def test_the_python_and_cxx_layers_carry_the_methods(repo_root):
    from fbus_ekf import BatchedFilter
    for m in ("set_depth_sensor", "correct_depth", "correct_depth_nis", "correct_depth_async"):
        assert callable(getattr(BatchedFilter, m))
    hdr = open(os.path.join(repo_root, "include", "fbus", "batched_filter.hpp")).read()
    for m in ("set_depth_sensor", "correct_depth", "correct_depth_dev", "correct_depth_async", "correct_depth_nis", "correct_depth_nis_dev"):
        assert f"void {m}(" in hdr, m
    assert "common.hpp:16" in open(os.path.join(repo_root, "include", "fbus_ekf.h")).read()


# ---- depth_ref against itself ---------------------------------------------------------------------------------------------------------------

def _state(n, seed):
    """a state with a NON-orthonormal carried rotation (what a run of predicts leaves) and a dense covariance"""
    rng = np.random.default_rng(seed)
    s = E.State(n)
    s.p, s.v = rng.uniform(-1, 1, 3), rng.normal(0, 0.1, 3)
    q = rng.normal(size=4)
    s.q = q / np.linalg.norm(q)
    s.R = E.q2R(s.q) + rng.normal(0, 1e-3, (3, 3))
    s.ba, s.bg, s.g = rng.normal(0, 0.05, 3), rng.normal(0, 0.002, 3), np.array([9.8, 0.0, 0.0])
    A = np.eye(n) + rng.normal(0, 0.05, (n, n))
    d = np.sqrt(E.Params(E.CPP, n).P0().diagonal())
    s.P = d[:, None] * (A @ A.T) * d[None, :]
    s.P = (s.P + s.P.T) / 2
    return s


@pytest.mark.parametrize("n", [18, 15])
def test_H_is_the_derivative_of_h(n):
    """central differences of depth_ref.h: p additively, R <- R (I +- [d]x) -- the injection's convention q <- q (x) dq(dtheta)"""
    a = depth_ref.unit(AXIS)
    for seed in range(4):
        s = _state(n, seed)
        H = depth_ref.H_row(s, n, a, LEVER)
        assert H.shape == (1, n)
        eps = 1e-6
        num = np.zeros(n)
        for i in range(3):
            d = np.zeros(3)
            d[i] = eps
            sp, sm = s.copy(), s.copy()
            sp.p, sm.p = s.p + d, s.p - d
            num[i] = (depth_ref.h(sp, a, 0.3, LEVER) - depth_ref.h(sm, a, 0.3, LEVER)) / (2 * eps)
            sp, sm = s.copy(), s.copy()
            sp.R, sm.R = s.R @ (np.eye(3) + E.skew(d)), s.R @ (np.eye(3) - E.skew(d))
            num[6 + i] = (depth_ref.h(sp, a, 0.3, LEVER) - depth_ref.h(sm, a, 0.3, LEVER)) / (2 * eps)
        # h is affine in p and in R: the central difference is exact up to the rounding of h itself, ~ eps_machine |h| / eps
        assert np.abs(H[0] - num).max() < 1e-9, np.abs(H[0] - num).max()
        assert np.all(H[0, 3:6] == 0) and np.all(H[0, 9:] == 0)


@pytest.mark.parametrize("n", [18, 15])
def test_the_three_covariance_forms_are_one_matrix(n):
    a = depth_ref.unit(AXIS)
    for seed in range(4):
        s = _state(n, 10 + seed)
        var = 10.0 ** (seed - 4)
        H = depth_ref.H_row(s, n, a, LEVER)
        lit, jos = s.copy(), s.copy()
        z = depth_ref.h(s, a, 0.3, LEVER) + 0.01
        r1 = depth_ref.correct_depth(lit, n, z, var, AXIS, 0.3, LEVER)
        r2 = depth_ref.correct_depth(jos, n, z, var, AXIS, 0.3, LEVER, joseph=True)
        assert r1 == r2 and r1[0] and r1[2] == 1
        rk = depth_ref.rank1(s.P, H, var)
        assert cov_rel_err_blockwise(lit.P[None], rk[None]) < 1e-12
        assert cov_rel_err_blockwise(jos.P[None], rk[None]) < 1e-12
        assert cov_rel_err_blockwise(jos.P[None], lit.P[None]) < 1e-12
        # the scalar identity: H P+ H' = var a / (a + var), a = H P- H'
        apri = (H @ s.P @ H.T).item()
        for post in (lit.P, jos.P, rk):
            assert abs((H @ post @ H.T).item() - var * apri / (apri + var)) < 1e-12 * apri
        # nis and S are the definition's
        assert abs(r1[3] - (apri + var)) < 1e-15 * r1[3] and abs(r1[1] - 0.01 ** 2 / r1[3]) < 1e-6 * r1[1]
        # the state moved along K: p by P_pJ H' res / S
        assert np.abs(lit.p - s.p - (s.P @ H.T).ravel()[0:3] * 0.01 / r1[3]).max() < 1e-9


def test_without_a_lever_the_theta_columns_are_exactly_zero():
    a = depth_ref.unit(AXIS)
    for n in (18, 15):
        s = _state(n, 3)
        for lever in (None, np.zeros(3)):
            H = depth_ref.H_row(s, n, a, depth_ref.lever_of(lever))
            assert np.all(H[0, 6:9] == 0.0) and np.array_equal(H[0, 0:3], a)


def test_untouched_filters_and_the_gate():
    s = _state(18, 5)
    for z, var, skip in ((np.nan, 1e-3, False), (np.inf, 1e-3, False), (0.1, 0.0, False), (0.1, -1.0, False), (0.1, np.nan, False),
                         (0.1, np.inf, False), (0.1, 1e-3, True)):
        t = s.copy()
        assert depth_ref.correct_depth(t, 18, z, var, AXIS, 0.0, LEVER, skip=skip)[:3] == (False, 0.0, 0)
        assert np.array_equal(t.P, s.P) and np.array_equal(t.p, s.p) and np.array_equal(t.q, s.q)
    t = s.copy()
    ok, nis, dof, S = depth_ref.correct_depth(t, 18, 5.0, 1e-3, AXIS, 0.0, LEVER, thr1=10.0)
    assert not ok and nis > 10.0 and dof == 1 and np.array_equal(t.P, s.P)


# ---- synth.depth -----------------------------------------------------------------------------------------------------------------------------

def test_two_shards_cut_inside_a_block_reproduce_the_unsharded_stream():
    B, cut = 2500, 1500                                   # the cut lies inside the second 1024-filter block
    nom, rot, _, _ = synth.initial_state(0, B, [1e-4] * 6, 18, with_cov=False)
    kw = dict(axis=AXIS, offset=0.4, lever=LEVER, noise=0.02)
    for step in (0, 3):
        whole = synth.depth(0, B, step, nom, rot, **kw)
        a = synth.depth(0, cut, step, nom[:cut], rot[:cut], **kw)
        b = synth.depth(cut, B, step, nom[cut:], rot[cut:], **kw)
        assert whole.shape == (B,) and whole.dtype == np.float64
        assert np.array_equal(np.concatenate([a, b]), whole)
    assert not np.array_equal(synth.depth(0, B, 0, nom, rot, **kw), synth.depth(0, B, 1, nom, rot, **kw))
    # the values are the model's: noise-free, z = axis . (p + R lever) + offset
    z0 = synth.depth(0, 64, 0, nom[:64], rot[:64], axis=AXIS, offset=0.4, lever=LEVER, noise=0.0)
    a = depth_ref.unit(AXIS)
    ref = [a @ (nom[b, 0:3] + rot[b].reshape(3, 3) @ LEVER) + 0.4 for b in range(64)]
    assert np.abs(z0 - ref).max() < 1e-15 * 4
    # rot_true = None: the rotation of the quaternion
    assert np.abs(synth.depth(0, 64, 0, nom[:64], None, axis=AXIS, offset=0.4, lever=LEVER, noise=0.0) - z0).max() < 1e-12
