"""CPU suite of the general linearised measurement update (include/fbus_ekf.h, fbus_ekf_correct_rows*; added under FBUS_ABI_VERSION 8
without a bump): tests/rows_ref.py -- the fp64 restatement the GPU suite holds the kernel to -- tied to the two restatements that exist
(depth_ref, velocity_ref) and to the identities between the forms of an m-row update; the Jacobians of the ready-made sensors of
fbus_ekf.rows against central differences through the injection; the four symbols and the layers above them; the untouched-lane rule; and
the domain of the re-acquisition cells of tests/test_rows_gpu.py."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import depth_ref
import ekf_oracle_np as E
import reacq_ref as Q
import rows_ref as W
import velocity_ref as V
from fbus_ekf import capi, rows
from support import state_batch
from util import COV_BLOCK_TOL, FLOOR_FACTOR, STATE_TOL, cov_rel_err_blockwise, state_rel_err

NEW = ["fbus_ekf_correct_rows", "fbus_ekf_correct_rows_dev", "fbus_ekf_correct_rows_nis", "fbus_ekf_correct_rows_nis_dev"]
MOUNT = V.tilted_mount()
LEVER = np.array([0.21, -0.08, 0.12])
GYRO = np.array([0.05, -0.11, 0.07])
VAR = np.array([1e-4, 4e-4, 2.5e-5])
AXIS, OFFSET, DLEVER, DVAR = np.array([0.12, -0.2, 1.0]), 0.4, np.array([0.11, -0.07, 0.05]), 1e-4
NB = 6


def states(n, dialect=1):
    prm, nom, rot, P, prev = state_batch(NB, dialect, n)
    return V.states_of((nom, rot, P, prev), n)


def same_update(a, b, ra, rb):
    """two states after the same update: state 1e-12, block-wise covariance 1e-12; applied, nis, dof, ln det S equal to 1e-12"""
    assert ra[0] == rb[0] and ra[2] == rb[2]
    assert abs(ra[1] - rb[1]) <= 1e-12 * abs(rb[1])
    lb = rb[3] if ra[2] > 1 else np.log(rb[3])          # (depth_ref returns S, the others ln det S)
    assert abs(ra[3] - lb) <= 1e-12 * max(1.0, abs(lb))
    for x, y in ((a.p, b.p), (a.v, b.v), (a.q, b.q), (a.ba, b.ba), (a.bg, b.bg), (a.g, b.g)):
        assert np.abs(x - y).max() <= 1e-12 * max(1.0, np.abs(y).max())
    assert cov_rel_err_blockwise(a.P[None], b.P[None]) <= 1e-12
    assert np.array_equal(a.R, b.R) and a.prev_id == b.prev_id


# ---- 1. the reference is tied to the two that exist -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [18, 15])
@pytest.mark.parametrize("joseph", [False, True])
def test_fed_the_depth_row_it_is_the_depth_restatement(n, joseph):
    a = depth_ref.unit(AXIS)
    for s in states(n):
        z = depth_ref.h(s, a, OFFSET, DLEVER) + 0.013
        t, u = s.copy(), s.copy()
        rb = depth_ref.correct_depth(u, n, z, DVAR, AXIS, OFFSET, DLEVER, joseph=joseph)
        ra = W.correct_rows(t, n, [z - depth_ref.h(s, a, OFFSET, DLEVER)], depth_ref.H_row(s, n, a, DLEVER), [DVAR], joseph=joseph)
        assert ra[0] and ra[2] == 1
        same_update(t, u, ra, rb)


@pytest.mark.parametrize("n", [18, 15])
@pytest.mark.parametrize("gyro", [None, GYRO])
def test_fed_the_velocity_rows_it_is_the_velocity_restatement(n, gyro):
    for joseph in (False, True):
        for s in states(n):
            h = V.h(s, MOUNT, LEVER, gyro)
            z = h + np.array([0.01, -0.02, 0.005])
            t, u = s.copy(), s.copy()
            rb = V.correct_velocity(u, n, z, VAR, gyro, MOUNT, LEVER, joseph=joseph)
            ra = W.correct_rows(t, n, z - h, V.H_rows(s, n, MOUNT, LEVER, gyro), VAR, joseph=joseph)
            assert ra[0] and ra[2] == 3
            same_update(t, u, ra, rb)


# ---- 2. one matrix in four forms --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [18, 15])
@pytest.mark.parametrize("m", [1, 2, 3])
def test_the_four_forms_are_one_matrix(n, m):
    rng = np.random.default_rng(100 * n + m)
    for s in states(n):
        H = rng.normal(0, 1, (m, n))
        assert (np.abs(H) > 0).all()                                     # dense: every column is in play
        # the noise at a tenth of, at, and at ten times the prior along each row: (I - K H) P, Joseph's form and P - U S^-1 U' are one
        # matrix in exact arithmetic and agree in double to eps x (H P H' / var), so the identity is checked where that factor is small
        hph = np.einsum("ki,ij,kj->k", H, s.P, H)
        var = hph * 10.0 ** rng.integers(-1, 2, m)
        res = rng.normal(0, 1, m) * np.sqrt(hph + var)
        lit, jos = s.copy(), s.copy()
        r1, r2 = W.correct_rows(lit, n, res, H, var), W.correct_rows(jos, n, res, H, var, joseph=True)
        assert r1 == r2 and r1[0] and r1[2] == m
        jn = W.joint(s.P, H, var)
        sq, dx, nis, lnd, ss = W.sequential(s.P, H, var, res)
        for a, b in ((lit.P, jn), (jos.P, jn), (jos.P, lit.P), (sq, jn), (sq, lit.P)):
            assert cov_rel_err_blockwise(a[None], b[None]) < 1e-12
        S = H @ s.P @ H.T + np.diag(var)
        assert abs(nis - res @ np.linalg.solve(S, res)) <= 1e-12 * nis and abs(nis - r1[1]) <= 1e-12 * nis
        assert abs(lnd - np.linalg.slogdet(S)[1]) <= 1e-12 * max(1.0, abs(lnd)) and abs(lnd - r1[3]) <= 1e-12 * max(1.0, abs(lnd))
        assert np.abs(ss - W.pivots_of(S)).max() <= 1e-12 * ss.max()
        Kres = s.P @ H.T @ np.linalg.solve(S, res)
        assert np.abs(dx - Kres).max() <= 1e-12 * np.abs(Kres).max()


def test_a_zero_row_adds_its_own_term_and_moves_nothing():
    n = 18
    s = states(n)[2]
    rng = np.random.default_rng(7)
    H = np.vstack([rng.normal(0, 1, (1, n)), np.zeros((1, n))])
    res, var = np.array([0.01, 0.03]), VAR[:2]
    one, two = s.copy(), s.copy()
    r1, r2 = W.correct_rows(one, n, res[:1], H[:1], var[:1]), W.correct_rows(two, n, res, H, var)
    assert r1[0] and r2[0] and r2[2] == 2
    assert abs(r2[1] - (r1[1] + res[1] ** 2 / var[1])) <= 1e-12 * r2[1]
    assert abs(r2[3] - (r1[3] + np.log(var[1]))) <= 1e-12 * abs(r2[3])
    assert cov_rel_err_blockwise(two.P[None], one.P[None]) <= 1e-12 and np.abs(two.p - one.p).max() <= 1e-15


# ---- 3. the Jacobians of fbus_ekf.rows --------------------------------------------------------------------------------------------------------

def _arrays(n):
    prm, nom, rot, P, prev = state_batch(NB, 1, n)
    rng = np.random.default_rng(3)
    rot = rot + rng.normal(0, 1e-3, rot.shape)           # a carried rotation is not orthonormal
    return torch.from_numpy(nom.copy()), torch.from_numpy(rot.copy())


def _expm(d):
    K = E.skew(d)
    a = np.linalg.norm(d)
    return np.eye(3) + np.sin(a) / a * K + (1 - np.cos(a)) / a ** 2 * (K @ K)


def _numeric(hfun, nom, rot, m, n, eps=1e-6):
    """central differences of h through the injection: p additively, R <- R exp([d]x)"""
    B = nom.shape[0]
    num = np.zeros((B, m, n))
    for i in range(3):
        d = np.zeros(3)
        d[i] = eps
        dp = torch.zeros_like(nom)
        dp[:, i] = eps
        num[:, :, i] = ((hfun(nom + dp, rot) - hfun(nom - dp, rot)) / (2 * eps)).numpy()
        R = rot.reshape(B, 3, 3).numpy()
        Rp, Rm = (torch.from_numpy((R @ x).reshape(B, 9)) for x in (_expm(d), _expm(d).T))
        num[:, :, 6 + i] = ((hfun(nom, Rp) - hfun(nom, Rm)) / (2 * eps)).numpy()
    return num


@pytest.mark.parametrize("n", [18, 15])
def test_the_ready_made_rows_are_the_derivatives_of_their_h(n):
    nom, rot = _arrays(n)
    assert nom.dtype == torch.float64
    B = nom.shape[0]
    zero3, zero1 = torch.zeros(B, 3, dtype=torch.float64), torch.zeros(B, 1, dtype=torch.float64)
    mw = np.array([0.22, -0.05, 0.43])
    p0 = nom[:, 0:3].numpy()
    R0 = rot.reshape(B, 3, 3).numpy()
    near = p0 + R0 @ LEVER + 0.3 * np.array([2.0, -1.0, 2.0]) / 3.0           # a beacon 0.3 m from the transponder
    cases = [("position_fix", 3, lambda a, r: rows.position_fix(a, r, zero3, LEVER, nstate=n)),
             ("position_fix no lever", 3, lambda a, r: rows.position_fix(a, r, zero3, nstate=n)),
             ("direction", 3, lambda a, r: rows.direction(a, r, zero3, mw, MOUNT, nstate=n)),
             ("direction no mount", 3, lambda a, r: rows.direction(a, r, zero3, mw, nstate=n)),
             ("range_to", 1, lambda a, r: rows.range_to(a, r, zero1, [4.0, -3.0, 1.5], LEVER, nstate=n)),
             ("range_to near", 1, lambda a, r: rows.range_to(a, r, zero1, near, LEVER, nstate=n)),
             ("range_to no lever", 1, lambda a, r: rows.range_to(a, r, zero1, [4.0, -3.0, 1.5], nstate=n))]
    for name, m, f in cases:
        res, H = f(nom, rot)
        assert res.shape == (B, m) and H.shape == (B, m, n) and res.dtype == torch.float64 and H.dtype == torch.float64, name
        num = _numeric(lambda a, r: -f(a, r)[0], nom, rot, m, n)          # z = 0: h = -res
        err = np.abs(H.numpy() - num).max()
        print(f"{name} N={n}: max |H - central differences| = {err:.2e}")
        assert err <= 1e-7, (name, err)
        Hn = H.numpy()
        assert (Hn[:, :, 3:6] == 0).all() and (Hn[:, :, 9:] == 0).all(), name
        if name.startswith("range_to near"):
            assert np.abs(np.linalg.norm(p0 + R0 @ LEVER - near, axis=1) - 0.3).max() < 1e-12
    # the models, as the docstrings state them
    z = torch.from_numpy(p0 + 0.5)
    res, _ = rows.position_fix(nom, rot, z, LEVER, nstate=n)
    assert np.abs(res.numpy() - (0.5 - R0 @ LEVER)).max() < 1e-12
    res, _ = rows.direction(nom, rot, zero3, mw, MOUNT, nstate=n)
    assert np.abs(-res.numpy() - np.einsum("bji,j->bi", R0, mw) @ MOUNT.T).max() < 1e-12          # h = C R' m_w
    # float32 in, float32 out
    r32_, H32 = rows.position_fix(nom.float(), rot.float(), z.float(), LEVER, nstate=n)
    assert r32_.dtype == torch.float32 and H32.dtype == torch.float32


# ---- 4. surface -------------------------------------------------------------------------------------------------------------------------------

def test_the_four_symbols_are_declared_exported_and_refuse_a_null_handle(repo_root):
    declared = capi.declared_symbols()
    lib = capi.load_library()
    for n in NEW:
        assert n in declared, n
        assert hasattr(lib, n), n
    assert "fbus_ekf_correct_rows_async" not in declared                  # (the header says why)
    assert capi.ABI_VERSION == 8 and lib.fbus_ekf_abi_version() == 8
    x = (C.c_float * 64)()
    var = (C.c_double * 3)(1.0, 1.0, 1.0)
    for fn in NEW[:2]:
        assert getattr(lib, fn)(None, 3, x, x, var, 0, None) == 1
        assert getattr(lib, fn)(None, 0, None, None, None, 2, None) == 1
    for fn in NEW[2:]:
        assert getattr(lib, fn)(None, 1, x, x, var, 0, None, None, None) == 1
    hdr = open(os.path.join(repo_root, "include", "fbus_ekf.h")).read()
    assert f"#define FBUS_ROWS_MAX {capi.ROWS_MAX}\n" in hdr and capi.ROWS_MAX == W.ROWS_MAX == 3


def test_the_kernel_builds_in_its_family_unit(repo_root):
    spec = importlib.util.spec_from_file_location("fbus_build_rows", os.path.join(repo_root, "fbus-ekf_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert any(h.endswith("ekf_rows.hpp") for h in b.HEADERS)            # a change of the kernel rebuilds the library
    assert any(h.endswith("ekf_sensor.hpp") for h in b.HEADERS)            # ... and so does one of the steps it shares
    csrc = os.path.join(repo_root, "fbus-ekf_amd", "csrc")
    units = [u for u in b.units() if u[0].endswith("_sensor")]
    assert sorted(u[0] for u in units) == ["f32_15_sensor", "f32_18_sensor", "f64_15_sensor", "f64_18_sensor"]
    assert {u[1] for u in units} == {os.path.join(csrc, "small_tu.hip")}
    # the family's branch of the unit source includes the header (over the steps the three sensor updates share): that unit instantiates the kernel
    code = b.FAMILIES["sensor"][0]
    tu = open(os.path.join(csrc, "small_tu.hip")).read()
    assert re.search(rf'#elif FBUS_TU_FAMILY == {code}\n(?:#include "ekf_\w+\.hpp"\n)*?#include "ekf_rows.hpp"\n', tu)
    assert all(f"-DFBUS_TU_FAMILY={code}" in u[2] for u in units)
    assert '#include "ekf_sensor.hpp"' in open(os.path.join(csrc, "ekf_rows.hpp")).read()
    main = open(os.path.join(csrc, "fbus_ekf.hip")).read()
    assert '#include "ekf_rows.hpp"' not in main                                  # ... and the host unit does not


def test_the_python_and_cxx_layers_carry_the_methods(repo_root):
    from fbus_ekf import BatchedFilter
    for m in ("correct_rows", "correct_rows_nis", "get_state_dev"):
        assert callable(getattr(BatchedFilter, m))
    assert not hasattr(BatchedFilter, "correct_rows_async")
    hdr = open(os.path.join(repo_root, "include", "fbus", "batched_filter.hpp")).read()
    for m in ("correct_rows", "correct_rows_dev", "correct_rows_nis", "correct_rows_nis_dev"):
        assert f"void {m}(" in hdr, m
    for f in ("position_fix", "direction", "range_to"):
        assert callable(getattr(rows, f)) and "h(x)" in getattr(rows, f).__doc__


# ---- 5. the untouched-lane rule ---------------------------------------------------------------------------------------------------------------

def test_untouched_filters_the_pivots_and_the_gate():
    n = 18
    s = states(n)[1]
    rng = np.random.default_rng(11)
    H, res = rng.normal(0, 1, (3, n)), np.array([0.01, -0.02, 0.005])
    nan3 = np.array([0.0, np.nan, 0.0])
    Hnan, Hinf = H.copy(), H.copy()
    Hnan[1, 7], Hinf[2, 16] = np.nan, np.inf
    for r, h, var, skip in ((res + nan3, H, VAR, False), (res + np.array([np.inf, 0, 0]), H, VAR, False), (res, Hnan, VAR, False),
                            (res, Hinf, VAR, False), (res, H, VAR * [1, 0, 1], False), (res, H, VAR * [1, 1, -1], False),
                            (res, H, VAR + nan3, False), (res, H, VAR * [np.inf, 1, 1], False), (res, H, VAR, True)):
        t = s.copy()
        assert W.correct_rows(t, n, r, h, var, skip=skip)[:3] == (False, 0.0, 0)
        assert np.array_equal(t.P, s.P) and np.array_equal(t.p, s.p) and np.array_equal(t.q, s.q)
    t = s.copy()
    ok, nis, dof, _ = W.correct_rows(t, n, res * 1e3, H, VAR, thr=10.0)
    assert not ok and nis > 10.0 and dof == 3 and np.array_equal(t.P, s.P)
    t = s.copy()
    ok, nis, dof, _ = W.correct_rows(t, n, res * 1e-2, H, VAR, thr=10.0)
    assert ok and nis <= 10.0 and dof == 3 and not np.array_equal(t.P, s.P)
    # a covariance that is not positive on the rows: a pivot <= 0 is not applied, whatever the gate; a NaN record: nis is NaN
    t = s.copy()
    t.P = -t.P * 1e3
    u = t.copy()
    ok, nis, dof, _ = W.correct_rows(u, n, res, H, VAR)
    assert not ok and dof == 3 and np.array_equal(u.P, t.P)
    t = s.copy()
    t.P = t.P * np.nan
    ok, nis, dof, _ = W.correct_rows(t, n, res[:2], H[:2], VAR[:2])
    assert not ok and np.isnan(nis) and dof == 2


# ---- the re-acquisition cells of the GPU suite --------------------------------------------------------------------------------------------------

def test_the_position_fix_ladder_stays_inside_the_domain_of_the_floor():
    """What test_rows_gpu.py's re-acquisition test bounds the fp32 kernel with is FLOOR_FACTOR x the figures of the fp64 reference rounded
    once to fp32.  Here, on the same rows and priors: that rounded reference is positive definite in every filter, is within 5 % of the
    posterior along the measured rows, and its state passes rule (e) -- the bound means something at every rung and does not gate the
    floor itself."""
    n = 18
    prm, nom, rot, P, prev = state_batch(Q.B_IND, 0, n)
    st0 = Q.as_record((nom, rot, P, prev), 32)
    res, H = W.fix_inputs(st0, 32, n)
    Hs = list(np.asarray(H, np.float64))
    for s in Q.LADDER:
        st = Q.grown(st0, s)
        (r_nom, _, r_P, _), app, _, _, _ = W.update_batch(st, n, res, H, W.FIX["var"], joseph=True)
        assert app.all()
        fl = Q.record_floor(r_P, Hs)
        pd = int((Q.min_eig(r_P.astype(np.float32)) > 0).sum())
        es, blk = state_rel_err(r_nom.astype(np.float32), r_nom, r_P)
        print(f"position_fix s = {s}: floor meas_err {fl['meas']:.2e} cov block-wise {fl['cov_block']:.2e}; rounded reference positive "
              f"definite in {pd} of {Q.B_IND}; rounded state {es:.2e} ({blk})")
        assert pd == Q.B_IND and fl["meas"] < 0.05
        for k in ("meas", "cov_block"):
            assert fl[k] <= max(COV_BLOCK_TOL, FLOOR_FACTOR * fl[k])
        assert es <= STATE_TOL
