"""GPU suite of the general linearised measurement update (include/fbus_ekf.h, fbus_ekf_correct_rows*; csrc/ekf_rows.hpp) against
tests/rows_ref.py, the fp64 restatement on ekf_oracle_np.State: parity of one update with dense rows (the body is
sensor_families.one_update, which the three streamed sensor updates share), the built-in sensors through the general door, a
free-running chain with the rows of fbus_ekf.rows evaluated on the device, a zero row, the refusals, and the re-acquisition ladder.
NIS / gate / untouched lanes, the four forms and a captured graph, per-filter variance, the likelihood sums and independence of the
neighbours are in tests/test_sensor_suite_gpu.py, once for the three updates.  B = 193 (three 64-filter tiles and a tile of one) unless
stated; the states are support.state_batch behind three predicts, so the carried rotation is the stale one."""
import ctypes as C

import numpy as np
import pytest
import torch

import depth_ref
import oracle_capi as oc
import reacq_ref as Q
import rows_ref as W
import velocity_ref as V
from fbus_ekf import BatchedFilter, capi, rows
from sensor_families import NIS_TOL, Rows, Velocity, ft, one_update, rel, rnd
from support import B_IND, DT, imu_of, markers_of, r32, same_state, state_batch, to_device
from util import (COV_BLOCK_TOL, COV_BLOCK_TOL_F64, F64_TOL, FLOOR_FACTOR, STATE_TOL, assert_parity, assert_window_parity,
                  cov_rel_err_blockwise, state_rel_err)

pytestmark = pytest.mark.gpu

B = B_IND
MOUNT, LEVER, VAR = Velocity.MOUNT, Velocity.LEVER, Velocity.VAR
ROWS = Rows(3)                                       # handle(): support.state_batch behind three predicts, and the rate sample


# ---- 0. parity of one update --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,n,m", [(d, n, m) for d in (32, 64) for n in (18, 15) for m in (1, 2, 3)])
def test_one_update_against_the_restatement(dtype, n, m):
    one_update(Rows(m), dtype, n, 1)


# ---- 1. the built-in sensors through the general door -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [32, 64])
def test_the_velocity_rows_through_the_general_door(dtype):
    n, dialect = 18, 1
    f, st0, w = ROWS.handle(B, dtype, n, dialect)
    g, st1, _ = ROWS.handle(B, dtype, n, dialect)
    with f, g:
        assert same_state(st0, st1)
        ss = V.states_of(st0, n)
        hx = np.array([V.h(s, MOUNT, LEVER, w[b]) for b, s in enumerate(ss)])
        z = rnd(hx + np.random.default_rng(5).normal(0, 1, (B, 3)) * np.sqrt(VAR), dtype)
        H = np.array([V.H_rows(s, n, MOUNT, LEVER, w[b]) for b, s in enumerate(ss)]).astype(ft(dtype))
        res = (z - hx).astype(ft(dtype))
        nis_r, dof_r = f.correct_rows_nis(res, H, VAR)
        g.set_velocity_sensor(MOUNT, LEVER)
        nis_v, dof_v = g.correct_velocity_nis(z, VAR, w)
        got_r, got_v = f.get_state(), g.get_state()
        assert f.applied().all() and g.applied().all() and (dof_r == 3).all() and (dof_v == 3).all()
    for s, b in zip(ss, range(B)):
        assert V.correct_velocity(s, n, z[b], VAR, w[b], MOUNT, LEVER)[0]
    ref = V.arrays_of(ss)
    assert_parity(got_r, ref, dtype, f"velocity rows through correct_rows f{dtype}")
    assert_parity(got_v, ref, dtype, f"correct_velocity f{dtype}")
    e = rel(nis_r.astype(np.float64), nis_v.astype(np.float64)).max()
    print(f"nis, correct_rows against correct_velocity: {e:.3e}")
    assert e <= NIS_TOL[dtype]


@pytest.mark.parametrize("dtype", [32, 64])
def test_the_depth_row_through_the_general_door(dtype):
    n, dialect = 15, 0
    AXIS, OFFSET, DLEVER, DVAR = Q.DEPTH["axis"], Q.DEPTH["offset"], Q.DEPTH["lever"], Q.DEPTH["var"]
    f, st0, _ = ROWS.handle(B, dtype, n, dialect)
    g, st1, _ = ROWS.handle(B, dtype, n, dialect)
    with f, g:
        assert same_state(st0, st1)
        ss = V.states_of(st0, n)
        a = depth_ref.unit(AXIS)
        hx = np.array([depth_ref.h(s, a, OFFSET, DLEVER) for s in ss])
        z = rnd(hx + np.random.default_rng(5).normal(0, 0.01, B), dtype)
        H = np.array([depth_ref.H_row(s, n, a, DLEVER) for s in ss]).astype(ft(dtype))
        res = (z - hx).astype(ft(dtype)).reshape(B, 1)
        nis_r, dof_r = f.correct_rows_nis(res, H, [DVAR])
        g.set_depth_sensor(AXIS, OFFSET, DLEVER)
        nis_d, dof_d = g.correct_depth_nis(z, DVAR)
        got_r, got_d = f.get_state(), g.get_state()
        assert f.applied().all() and g.applied().all() and (dof_r == 1).all() and (dof_d == 1).all()
    for b, s in enumerate(ss):
        assert depth_ref.correct_depth(s, n, float(z[b]), DVAR, AXIS, OFFSET, DLEVER)[0]
    ref = V.arrays_of(ss)
    assert_parity(got_r, ref, dtype, f"depth row through correct_rows f{dtype}")
    assert_parity(got_d, ref, dtype, f"correct_depth f{dtype}")
    e = rel(nis_r.astype(np.float64), nis_d.astype(np.float64)).max()
    print(f"nis, correct_rows against correct_depth: {e:.3e}")
    assert e <= NIS_TOL[dtype]


# ---- 2. a free-running chain ----------------------------------------------------------------------------------------------------------------------

def skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def fix_rows_np(ref, n):
    """h and H of rows.position_fix on get_state()-shaped fp64 arrays, written from its docstring"""
    nom, R = np.asarray(ref[0], np.float64), np.asarray(ref[1], np.float64).reshape(-1, 3, 3)
    H = np.zeros((len(nom), 3, n))
    H[:, :, 0:3] = np.eye(3)
    H[:, :, 6:9] = -R @ skew(LEVER)
    return nom[:, 0:3] + R @ LEVER, H


def range_rows_np(ref, n, beacon):
    nom, R = np.asarray(ref[0], np.float64), np.asarray(ref[1], np.float64).reshape(-1, 3, 3)
    d = nom[:, 0:3] + R @ LEVER - beacon
    r = np.linalg.norm(d, axis=1)
    e = d / r[:, None]
    H = np.zeros((len(nom), 1, n))
    H[:, 0, 0:3] = e
    H[:, 0, 6:9] = -np.einsum("bi,bij->bj", e, R @ skew(LEVER))
    return r[:, None], H


@pytest.mark.parametrize("n,dialect", [(18, 1), (15, 0)])
def test_a_chain_of_predicts_position_fixes_ranges_and_pose_updates(n, dialect):
    """12 x (predict_n K = 7, correct_rows with rows.position_fix evaluated on the device from get_state_dev), a stacked pose update every
    fourth step and a rows.range_to update (m = 1) every third, free-running against the oracle + rows_ref"""
    K, STEPS = 7, 12
    BEACON, RVAR = np.array([4.0, -3.0, 1.5]), 1e-4
    prm, nom, rot, P, prev = state_batch(B, dialect, n)
    orc = oc.Oracle(dialect, n)
    ref = [np.array(nom), np.array(rot), np.array(P), np.array(prev)]
    rng = np.random.default_rng(9)
    worst = []
    with BatchedFilter(B, prm, device=0, dtype=32, nstate=n) as f:
        f.set_state(nom, rot, P, prev)
        for step in range(STEPS):
            acc, gyr = imu_of(0, B, step * K, K, nom)
            f.predict_n(acc, gyr, np.repeat(DT, K))
            for k in range(K):
                orc.predict(*ref, acc[k], gyr[k], DT)
            if step % 4 == 3:
                ids, pos, quat = markers_of(0, B, step, 4, nom, prm)
                f.correct(ids, pos, quat, capi.MODE_STACKED)
                orc.correct(*ref, ids, pos, quat, oc.STACKED)
            if step % 3 == 2:
                hr, Hr = range_rows_np(ref, n, BEACON)
                zr = r32(hr + rng.normal(0, 0.01, (B, 1)))
                dn, dr = f.get_state_dev()
                f.correct_rows(*rows.range_to(dn, dr, to_device(zr, np.float32), BEACON, LEVER, nstate=n), [RVAR])
                assert f.applied().all()
                out = W.update_batch(ref, n, zr - hr, Hr, [RVAR])
                assert out[1].all()
                ref = list(out[0])
            hx, Hx = fix_rows_np(ref, n)
            z = r32(hx + rng.normal(0, 1, (B, 3)) * np.sqrt(VAR))
            dn, dr = f.get_state_dev()
            dres, dH = rows.position_fix(dn, dr, to_device(z, np.float32), LEVER, nstate=n)
            assert dres.is_cuda and dres.dtype == torch.float32 and dH.shape == (B, 3, n)
            f.correct_rows(dres, dH, VAR)
            after = f.get_state()
            assert f.applied().all()
            out = W.update_batch(ref, n, z - hx, Hx, VAR)
            assert out[1].all()
            ref = list(out[0])
            # the update shrinks the variance along its own rows: diag(H P+ H') < var (H P+ H' = R - R S^-1 R for the joint update)
            Hd = dH.cpu().numpy().astype(np.float64)
            worst.append((np.einsum("bki,bij,bkj->bk", Hd, np.asarray(after[2], np.float64), Hd) / VAR).max())
        got = f.get_state()
    for step, w in enumerate(worst):
        print(f"step {step}: max diag(H P+ H') / var = {w:.6f}")
    try:
        assert_window_parity(got, ref, f"rows chain N={n} dialect {dialect}", dialect, n)
    finally:
        for step, w in enumerate(worst):
            assert w < 1.0, (step, w)


# ---- 3. a zero row -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [32, 64])
def test_a_zero_row_adds_its_term_to_nis_and_moves_nothing(dtype):
    n = 18
    f, st0, _ = ROWS.handle(B, dtype, n, 1)
    g, _, _ = ROWS.handle(B, dtype, n, 1)
    with f, g:
        res, H, var, _ = Rows(2).dense(st0, dtype)
        H[:, 1, :] = 0
        nis2, dof2 = f.correct_rows_nis(res, H, var)
        nis1, dof1 = g.correct_rows_nis(res[:, :1].copy(), H[:, :1].copy(), var[:, :1].copy())
        got2, got1 = f.get_state(), g.get_state()
        assert f.applied().all() and g.applied().all() and (dof2 == 2).all() and (dof1 == 1).all()
    ref1 = W.update_batch(st0, n, res[:, :1], H[:, :1], var[:, :1])[0]
    assert_parity(got2, ref1, dtype, f"a zero second row f{dtype}: the m = 2 call against the m = 1 restatement")
    assert_parity(got1, ref1, dtype, f"a zero second row f{dtype}: the m = 1 call")
    want = nis1.astype(np.float64) + res[:, 1].astype(np.float64) ** 2 / var[:, 1]
    assert rel(nis2.astype(np.float64), want).max() <= NIS_TOL[dtype]


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------------------------

def test_refused_calls_launch_nothing():
    n = 18
    f, st0, _ = ROWS.handle(B, 32, n, 1)
    with f:
        res, H, var, _ = ROWS.dense(st0, 32)
        dr, dH, dv = to_device(res), to_device(H), to_device(var)
        last = lambda: f._lib.fbus_ekf_last_error(f._h).decode()
        vp = lambda t: C.c_void_p(t.data_ptr())
        hp = lambda a: a.ctypes.data_as(C.c_void_p)
        forms = (("fbus_ekf_correct_rows", hp, (res, H, var), ()), ("fbus_ekf_correct_rows_dev", vp, (dr, dH, dv), ()),
                 ("fbus_ekf_correct_rows_nis", hp, (res, H, var), (None, None)), ("fbus_ekf_correct_rows_nis_dev", vp, (dr, dH, dv), (None, None)))
        for name, p, (a, h, v), tail in forms:
            fn = getattr(f._lib, name)
            for m in (0, 4, -1):
                assert fn(f._h, m, p(a), p(h), p(v), 1, None, *tail) == 1
                assert name + ":" in last() and "m = " in last(), last()
            for args in ((None, p(h), p(v)), (p(a), None, p(v)), (p(a), p(h), None)):
                assert fn(f._h, 3, *args, 1, None, *tail) == 1
                assert name + ":" in last() and "NULL" in last(), last()
            assert fn(f._h, 3, p(a), p(h), p(v), 2, None, *tail) == 1
            assert name + ":" in last() and "var_per_filter" in last()
            assert fn(f._h, 0, None, None, None, 2, None, *tail) == 1 and "m = " in last()          # the order of the checks
            assert fn(None, 3, p(a), p(h), p(v), 1, None, *tail) == 1
        # the Python layer's own checks
        with pytest.raises(ValueError):
            f.correct_rows(res, H[:, :2], var)
        with pytest.raises(ValueError):
            f.correct_rows(res, H, var[:, :2])
        with pytest.raises(ValueError):
            f.correct_rows(dr, dH.double(), dv)
        # inside a capture: the host forms
        f._check(f._lib.fbus_ekf_graph_begin(f._h), "graph_begin")
        try:
            assert f._lib.fbus_ekf_correct_rows(f._h, 3, hp(res), hp(H), hp(var), 1, None) == 1
            assert "fbus_ekf_correct_rows:" in last() and "graph_begin" in last()
            assert f._lib.fbus_ekf_correct_rows_nis(f._h, 3, hp(res), hp(H), hp(var), 1, None, None, None) == 1
            assert "fbus_ekf_correct_rows_nis:" in last()
        finally:
            gid = C.c_int(-1)
            f._lib.fbus_ekf_graph_end(f._h, C.byref(gid))
        f.sync()
        assert same_state(st0, f.get_state()) and (f.applied() == 0).all()
        f.correct_rows(dr, dH, dv)                                    # ... and the handle is as good as new
        f.sync()
        assert f.applied().all() and not same_state(st0, f.get_state())


# ---- 5. re-acquisition ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,n,form", [(32, 18, "a"), (64, 15, "b")])
def test_position_fix_rows_against_a_grown_prior(dtype, n, form):
    """rows.position_fix (m = 3) against the prior grown by s = 1, 10, 100, judged as tests/test_reacquisition_gpu.py judges the velocity
    update: fp32 records by its rule (a), fp64 by (b), the state by (e).  (tests/test_rows_cpu.py checks that the rounded fp64 reference
    stays inside the domain of rule (a) on these inputs.)"""
    what = f"position_fix f{dtype} N={n}"
    f, st0, _ = ROWS.handle(B, dtype, n, 0)
    with f:
        res, H = W.fix_inputs(st0, dtype, n)
        Hs = list(np.asarray(H, np.float64))
        var = W.FIX["var"]
        for s in Q.LADDER:
            st = Q.grown(st0, s)
            f.set_state(*st)
            f.correct_rows_nis(res, H, var)
            got, app = f.get_state(), f.applied()
            assert app.all(), (what, s)
            (r_nom, _, r_P, r_prev), r_app = W.update_batch(st, n, res, H, var, joseph=True)[:2]
            assert r_app.all()
            g_P = np.asarray(got[2], np.float64)
            e = {"meas": Q.meas_err(g_P, r_P, Hs), "cov_block": cov_rel_err_blockwise(g_P, r_P)}
            fl = Q.record_floor(r_P, Hs)
            if form == "a":
                bound = {k: max(COV_BLOCK_TOL, FLOOR_FACTOR * fl[k]) for k in e}
                base = {k: FLOOR_FACTOR * fl[k] for k in e}
            else:
                alt = W.update_batch(st, n, res, H, var, joseph=False)[0][2]
                base = {"meas": Q.meas_err(alt, r_P, Hs), "cov_block": cov_rel_err_blockwise(alt, r_P)}
                bound = {"meas": max(F64_TOL, 2 * base["meas"]), "cov_block": max(COV_BLOCK_TOL_F64, 2 * base["cov_block"])}
            es, blk = state_rel_err(got[0], r_nom, r_P)
            pd = int((Q.min_eig(g_P) > 0).sum())
            of = {"a": "its 1.5 x floor", "b": "(I - K H) P vs Joseph"}[form]
            print(f"[reacq] {what} s={s} ({form}): meas_err {e['meas']:.2e} (bound {bound['meas']:.2e}, {of} {base['meas']:.2e}, "
                  f"fp32-record floor {fl['meas']:.2e}, kernel / floor {e['meas'] / fl['meas']:.2f})  cov block-wise {e['cov_block']:.2e} "
                  f"(bound {bound['cov_block']:.2e}, {of} {base['cov_block']:.2e}, kernel / floor {e['cov_block'] / fl['cov_block']:.2f})  "
                  f"state {es:.2e} ({blk})  positive definite {pd} of {B}")
            assert e["meas"] <= bound["meas"], f"{what} s={s}: meas_err {e['meas']:.3g} > {bound['meas']:.3g}"
            assert e["cov_block"] <= bound["cov_block"], f"{what} s={s}: block-wise covariance rel err {e['cov_block']:.3g} > {bound['cov_block']:.3g}"
            assert np.array_equal(got[2], np.swapaxes(got[2], 1, 2)), f"{what} s={s}: covariance not exactly symmetric"
            assert pd == B, f"{what} s={s}: P positive definite in {pd} of {B} filters"
            assert es <= (STATE_TOL if dtype == 32 else F64_TOL), f"{what} s={s}: state rel err {es:.3g} in block {blk}"
            assert np.array_equal(got[3], r_prev), f"{what} s={s}: prev marker id"
