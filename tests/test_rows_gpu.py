"""GPU suite of the general linearised measurement update (include/fbus_ekf.h, fbus_ekf_correct_rows*; csrc/ekf_rows.hpp) against
tests/rows_ref.py, the fp64 restatement on ekf_oracle_np.State: parity of one update with dense rows, the built-in sensors through the
general door, a free-running chain with the rows of fbus_ekf.rows evaluated on the device, NIS / gate / untouched lanes, the four forms
and a captured graph, per-filter variance, the likelihood sums, independence of the neighbours, a zero row, the refusals, and the
re-acquisition ladder.  B = 193 (three 64-filter tiles and a tile of one) unless stated; the states are support.state_batch behind three
predicts, so the carried rotation is the stale one."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import depth_ref
import oracle_capi as oc
import reacq_ref as Q
import rows_ref as W
import velocity_ref as V
from fbus_ekf import BatchedFilter, capi, rows
from support import (B_IND, DT, imu_of, markers_of, permutation, poison_set, poisoned_state, r32, ragged_cut, same_rows, same_state,
                     state_batch, to_device)
from util import (COV_BLOCK_TOL, COV_BLOCK_TOL_F64, F64_TOL, FLOOR_FACTOR, STATE_TOL, assert_parity, assert_window_parity,
                  cov_rel_err_blockwise, state_rel_err)

pytestmark = pytest.mark.gpu

B = B_IND
MOUNT = V.tilted_mount()
LEVER = np.array([0.21, -0.08, 0.12])
VAR = np.array([1e-4, 4e-4, 2.5e-5])
RATIO = np.array([300.0, 1000.0, 3000.0])            # H P H' / var of the dense cases, row by row
NAMES = ("nominal", "rot", "P", "prev")
NIS_TOL = {32: 1e-4, 64: 1e-9}                       # the velocity suite's: in fp32 S inherits the covariance gate


def rnd(a, dtype):
    return r32(a) if dtype == 32 else np.asarray(a, np.float64)


def ft(dtype):
    return np.float32 if dtype == 32 else np.float64


def rel(a, b):
    return np.abs(a - b) / np.abs(b)


def carried(nB, dtype, n, dialect, seed_off=0):
    """a handle whose records hold a state of support.state_batch behind three predicts (the carried rotation is the stale one);
    returns (handle, its state as get_state() gives it, the rate sample that goes with a reading)"""
    prm, nom, rot, P, prev = state_batch(nB, dialect, n, seed_off=seed_off)
    f = BatchedFilter(nB, prm, device=0, dtype=dtype, nstate=n)
    f.set_state(nom, rot, P, prev)
    a, w = imu_of(seed_off, seed_off + nB, 0, 4, nom)
    for k in range(3):
        f.predict(a[k], w[k], DT)
    return f, f.get_state(), w[3]


def dense(st0, dtype, n, m, seed=5):
    """dense rows, every column non-zero, scaled by the prior's sigmas so that every block of the state is in play; a variance per
    filter and row that puts H P H' / var at RATIO; a residual of the size of S.  All representable in the record type (var is double).
    -> res (B, m), H (B, m, n), var (B, m), hph (B, m)"""
    P = np.asarray(st0[2], np.float64)
    nB = len(P)
    rng = np.random.default_rng(seed + 10 * m)
    d = 1.0 / np.sqrt(np.median(np.einsum("bii->bi", P), axis=0))
    H = rng.uniform(0.3, 1.0, (nB, m, n)) * rng.choice([-1.0, 1.0], (nB, m, n)) * d
    H = rnd(H, dtype)
    hph = np.einsum("bki,bij,bkj->bk", H, P, H)
    var = hph / RATIO[:m]
    res = rnd(rng.normal(0, 1, (nB, m)) * np.sqrt(hph + var), dtype)
    return res.astype(ft(dtype)), H.astype(ft(dtype)), var, hph


def outs(f, nis=None, dof=None):
    d = dict(zip(NAMES, f.get_state()), applied=f.applied())
    if nis is not None:
        d.update(nis=nis, dof=dof)
    return d


# ---- 1. parity of one update --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,n,m", [(d, n, m) for d in (32, 64) for n in (18, 15) for m in (1, 2, 3)])
def test_one_update_against_the_restatement(dtype, n, m):
    f, st0, _ = carried(B, dtype, n, 1)
    with f:
        res, H, var, hph = dense(st0, dtype, n, m)
        assert (H != 0).all()
        ratio = hph / var
        assert ratio.min() >= 100 and ratio.max() <= 1e4, (ratio.min(), ratio.max())          # in the hundreds to thousands, every row
        nis, dof = f.correct_rows_nis(res, H, var)
        got, app = f.get_state(), f.applied()
    assert app.all() and (dof == m).all()
    for joseph in (False, True):
        ref, rapp, rnis, rdof, _ = W.update_batch(st0, n, res, H, var, joseph=joseph)
        assert rapp.all()
        print(f"nis rel err {rel(nis.astype(np.float64), rnis).max():.3e}")
        assert_parity(got, ref, dtype, f"correct_rows f{dtype} N={n} m={m} joseph {joseph}")
        assert rel(nis.astype(np.float64), rnis).max() <= NIS_TOL[dtype]
    assert np.array_equal(got[1], st0[1]) and np.array_equal(got[3], st0[3])          # R and prev_id are not written
    assert not np.array_equal(got[0], st0[0])
    if n == 15:
        assert np.array_equal(got[0][:, 16:19], st0[0][:, 16:19])                      # no gravity state: g stays


# ---- 2. the built-in sensors through the general door -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [32, 64])
def test_the_velocity_rows_through_the_general_door(dtype):
    n, dialect = 18, 1
    f, st0, w = carried(B, dtype, n, dialect)
    g, st1, _ = carried(B, dtype, n, dialect)
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
    f, st0, _ = carried(B, dtype, n, dialect)
    g, st1, _ = carried(B, dtype, n, dialect)
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


# ---- 3. one filter, one full tile -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nB", [1, 64])
def test_one_filter_and_one_full_tile(nB):
    f, st0, _ = carried(nB, 32, 18, 1)
    with f:
        res, H, var, _ = dense(st0, 32, 18, 3)
        f.correct_rows(res, H, var)
        got = f.get_state()
        assert f.applied().all()
    assert_parity(got, W.update_batch(st0, 18, res, H, var)[0], 32, f"correct_rows B = {nB}")


# ---- 4. a free-running chain ----------------------------------------------------------------------------------------------------------------------

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


# ---- 5. NIS, gate, untouched lanes --------------------------------------------------------------------------------------------------------------

KINDS = {1: "skip", 2: "NaN res", 3: "inf res", 4: "NaN in H", 5: "var 0", 6: "var < 0", 7: "var inf", 8: "var NaN"}


def mixed_inputs(st0, dtype, n=18, m=3):
    """dense rows with a tail of outliers on one residual, and the lanes that must stay untouched, one kind per lane group
    (b % 16 == 3, 7, 11, 15 and b % 32 == 5, 13, 21, 29): 12 x 4 + 6 x 4 = 72 of the 193 lanes.  -> (res, H, var, skip, kinds)"""
    nB = len(st0[0])
    b = np.arange(nB)
    res, H, var, hph = dense(st0, dtype, n, m)
    res, H, var = res.copy(), H.copy(), var.copy()
    out = b % 5 == 2
    res[out, 1 % m] += (6.0 * np.sqrt(hph[out, 1 % m])).astype(res.dtype)          # outliers for the gate
    kinds = np.zeros(nB, int)
    for k, sel in ((1, b % 16 == 3), (2, b % 16 == 7), (3, b % 16 == 11), (4, b % 16 == 15), (5, b % 32 == 5), (6, b % 32 == 13),
                   (7, b % 32 == 21), (8, b % 32 == 29)):
        kinds[sel] = k
    skip = (kinds == 1).astype(np.uint8)
    res[kinds == 2, b[kinds == 2] % m] = np.nan
    res[kinds == 3, b[kinds == 3] % m] = np.inf
    w = b[kinds == 4]
    H[w, w % m, (5 * w) % n] = np.nan                                             # a single entry
    var[kinds == 5, b[kinds == 5] % m] = 0.0
    var[kinds == 6, b[kinds == 6] % m] = -1e-4
    var[kinds == 7, b[kinds == 7] % m] = np.inf
    var[kinds == 8, b[kinds == 8] % m] = np.nan
    return res, H, var, skip, kinds


def gate_between(nis, share=0.9):
    """a threshold strictly between two neighbouring values of the sorted finite nis"""
    v = np.sort(nis[np.isfinite(nis) & (nis > 0)].astype(np.float64))
    i = int(share * len(v))
    assert v[i - 1] < v[i]
    return 0.5 * (v[i - 1] + v[i])


@pytest.mark.parametrize("dtype", [32, 64])
def test_nis_gate_and_untouched_lanes(dtype):
    n, m = 18, 3
    f, st0, _ = carried(B, dtype, n, 1)
    with f:
        res, H, var, skip, kinds = mixed_inputs(st0, dtype)
        nis0, _ = f.correct_rows_nis(res, H, var, skip)              # ungated: the device's own nis
    thr = gate_between(nis0)
    f, st1, _ = carried(B, dtype, n, 1)
    with f:
        assert same_state(st0, st1)
        f.set_gate([np.inf, np.inf, np.inf])                         # m entries: no thr[m]
        for call in (lambda: f.correct_rows(res, H, var, skip), lambda: f.correct_rows_nis(to_device(res), to_device(H), to_device(var))):
            with pytest.raises(capi.FbusError) as e:
                call()
            assert e.value.code == 1 and "fbus_ekf_correct_rows" in str(e.value) and "gate table" in str(e.value)
        f.sync()
        assert same_state(st0, f.get_state())
        f.set_gate([np.inf, np.inf, np.inf, thr])
        nis, dof = f.correct_rows_nis(res, H, var, skip)
        got, app = f.get_state(), f.applied()
    assert np.array_equal(nis, nis0)
    usable = kinds == 0
    assert (~usable).sum() == 72 and all((kinds == k).sum() >= 6 for k in KINDS)
    rejected = usable & ~(nis.astype(np.float64) <= thr)
    applied = usable & ~rejected
    assert rejected.sum() >= 10 and np.array_equal(app.astype(bool), applied)
    assert np.array_equal(dof, m * usable.astype(np.int32))          # rejected m; every unusable kind 0
    assert (nis[~usable] == 0).all()
    assert same_state(st0, got, rows=np.nonzero(~applied)[0])       # record bytes unchanged
    ref, rapp, rnis, rdof, _ = W.update_batch(st0, n, res, H, var, skip=skip)
    assert np.array_equal(rapp, usable) and np.array_equal(rdof, dof)
    print(f"nis rel err {rel(nis.astype(np.float64)[usable], rnis[usable]).max():.3e}")
    assert rel(nis.astype(np.float64)[usable], rnis[usable]).max() <= NIS_TOL[dtype]
    sel = np.nonzero(applied)[0]
    assert_parity([x[sel] for x in got], [x[sel] for x in ref], dtype, f"gated correct_rows f{dtype}: the applied lanes")


# ---- 6. forms -------------------------------------------------------------------------------------------------------------------------------------

def chi2_gate(m):
    return {1: 3.84, 2: 5.99, 3: 7.81}[m]              # chi-square, 95 %: the outlier tail lies above it


def test_every_form_and_a_captured_graph_hold_the_same_bits():
    dtype, n, m = 32, 18, 3
    res = None
    got = {}
    for form in ("host", "dev", "nis", "nis null", "nis dev", "graph"):
        f, st0, _ = carried(B, dtype, n, 1)
        with f:
            if res is None:
                res, H, var, skip, _ = mixed_inputs(st0, dtype)
            f.set_gate([np.inf] * m + [chi2_gate(m)])
            dr, dH, dv, ds = to_device(res), to_device(H), to_device(var), to_device(skip)
            if form == "host":
                f.correct_rows(res, H, var, skip)
            elif form == "dev":
                f.correct_rows(dr, dH, dv, ds)
            elif form == "nis":
                f.correct_rows_nis(res, H, var, skip)
            elif form == "nis null":
                vp = lambda t: C.c_void_p(t.data_ptr())
                assert f._lib.fbus_ekf_correct_rows_nis_dev(f._h, m, vp(dr), vp(dH), vp(dv), 1, vp(ds), None, None) == 0
            elif form == "nis dev":
                f.correct_rows_nis(dr, dH, dv, ds)
            else:
                gid = f.graph_capture(lambda: f.correct_rows(dr, dH, dv, ds))
                f.sync()
                assert same_state(st0, f.get_state())                  # capturing launched nothing
                f.graph_launch(gid)
            f.sync()
            got[form] = outs(f)
    assert 0 < got["host"]["applied"].sum() < B
    for form in got:
        assert same_rows(got["host"], got[form]), form


# ---- 7. per-filter variance -----------------------------------------------------------------------------------------------------------------------

def test_a_per_filter_variance_is_the_scalar_set_of_a_handle_of_its_own():
    dtype, n, m = 32, 18, 3
    f, st0, _ = carried(B, dtype, n, 0)
    with f:
        res, H, var, _ = dense(st0, dtype, n, m)
        f.correct_rows(res, H, var)
        whole = outs(f)
    picks = (0, 63, 64, 100, 192)
    for b in picks:
        f, _, _ = carried(B, dtype, n, 0)
        with f:
            f.correct_rows(res, H, var[b])                           # the m scalars of filter b for every filter
            one = outs(f)
        assert same_rows(whole, one, [b], [b]), b
    other = [p for p in picks if p != b]
    assert not same_rows(whole, one, other, other)                    # (the variance does matter)


# ---- 8. likelihood --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [32, 64])
def test_the_likelihood_sums(dtype):
    """two calls, m = 3 with gated and untouched lanes and then m = 1 on every lane, the sums against the restatement's ln det S"""
    n = 18
    got = {}
    for lik in (False, True):
        f, st0, _ = carried(B, dtype, n, 1)
        with f:
            res, H, var, skip, kinds = mixed_inputs(st0, dtype)
            f.set_gate([np.inf, 1e9, np.inf, chi2_gate(3)])
            if lik:
                f.loglik_enable()
                assert all((x == 0).all() for x in f.loglik())
            nis3, dof3 = f.correct_rows_nis(res, H, var, skip)
            st1, app3 = f.get_state(), f.applied().astype(bool)
            res1, H1, var1, _ = dense(st1, dtype, n, 1, seed=23)
            nis1, dof1 = f.correct_rows_nis(res1, H1, var1)
            got[lik] = outs(f, np.stack([nis3, nis1]), np.stack([dof3, dof1]))
            app1 = f.applied().astype(bool)
            if lik:
                ll, nrows, napp, nrej = f.loglik()
    assert same_rows(got[False], got[True])                          # the sums change no record, flag or output
    rej3 = (kinds == 0) & ~app3
    assert app3.sum() >= 80 and rej3.sum() >= 10 and app1.all()          # (121 lanes are usable, a fifth of them outliers)
    assert np.array_equal(nrows, 3 * app3.astype(np.int64) + 1) and np.array_equal(napp, app3.astype(np.int32) + 1)
    assert np.array_equal(nrej, rej3.astype(np.int32))
    lnd3 = W.update_batch(st0, n, res, H, var, thr=chi2_gate(3), skip=skip)[4]
    lnd1 = W.update_batch(st1, n, res1, H1, var1)[4]
    want = -0.5 * (nis1.astype(np.float64) + lnd1 + math.log(2 * math.pi))
    want[app3] += -0.5 * (nis3.astype(np.float64)[app3] + lnd3[app3] + 3 * math.log(2 * math.pi))
    err = np.abs(ll - want).max()
    print(f"f{dtype}: max |ll - sum (-1/2)(nis + ln det S + m ln 2 pi)| = {err:.3e}")
    assert err <= 1e-9 + NIS_TOL[dtype]


# ---- 9, 10. independence --------------------------------------------------------------------------------------------------------------------------

def _job(dtype=32, n=18):
    f, st0, _ = carried(B, dtype, n, 1)
    f.close()
    return (st0,) + mixed_inputs(st0, dtype)[:4]


def _run(st, res, H, var, skip, dtype=32, n=18, dev=False):
    """one gated update on a fresh handle holding exactly the state st; also returns the records as they were before it"""
    nB = len(st[0])
    dv = (lambda x: to_device(x)) if dev else (lambda x: x)
    with BatchedFilter(nB, capi.default_params(1), device=0, dtype=dtype, nstate=n) as f:
        f.set_state(*st)
        before = dict(zip(NAMES, f.get_state()))
        f.set_gate([np.inf] * 3 + [chi2_gate(3)])
        nis, dof = f.correct_rows_nis(dv(res), dv(H), dv(var), dv(skip))
        f.sync()
        if dev:
            nis, dof = nis.cpu().numpy(), dof.cpu().numpy()
        return outs(f, nis, dof), before


def test_a_filter_is_itself_wherever_it_stands():
    st0, res, H, var, skip = _job()
    v0, _ = _run(st0, res, H, var, skip)
    assert 0 < v0["applied"].sum() < B
    pi = permutation()
    assert same_rows(v0, _run([x[pi] for x in st0], res[pi], H[pi], var[pi], skip[pi])[0], rows=pi)
    # two handles cut inside a tile; the second reads SLICES of the whole job's device arrays, off the 16-byte boundary
    dr, dH, dv, ds = to_device(res), to_device(H), to_device(var), to_device(skip)
    for part in ragged_cut():
        lo, hi = part[0], part[-1] + 1
        if lo:
            assert dr[lo:hi].data_ptr() % 16 != 0 and dH[lo:hi].data_ptr() % 16 != 0
        assert same_rows(v0, _run([x[part] for x in st0], dr[lo:hi], dH[lo:hi], dv[lo:hi], ds[lo:hi], dev=True)[0], rows=part)


def test_a_clean_lane_among_broken_records_keeps_its_bits():
    st0, res, H, var, skip = _job()
    v0, _ = _run(st0, res, H, var, skip)
    S, form = poison_set()
    nom, rot, P = poisoned_state(st0[0], st0[1], st0[2], S, form)
    rr = res.copy()
    rr[S[form == 3], 0] = np.nan                                     # form (d): the input is broken, not the record
    out, before = _run([nom.astype(np.float32), rot.astype(np.float32), P.astype(np.float32), st0[3]], rr, H, var, skip)
    clean = np.setdiff1d(np.arange(B), S)
    assert 100 in clean and len(np.intersect1d(clean, np.arange(64, 128))) == 1          # a whole wave but one lane
    assert same_rows(v0, out, clean, clean)
    # a record of NaN (a: nis is NaN), one with a negated covariance (c: no positive pivot) and a broken residual (d) are not applied;
    # whatever is not applied keeps its bytes
    for k in (0, 2, 3):
        assert (out["applied"][S[form == k]] == 0).all(), k
    kept = S[out["applied"][S] == 0]
    assert len(kept) >= len(S) * 3 // 5
    assert same_rows(before, {k: out[k] for k in NAMES}, kept, kept)


# ---- 11. a zero row -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [32, 64])
def test_a_zero_row_adds_its_term_to_nis_and_moves_nothing(dtype):
    n = 18
    f, st0, _ = carried(B, dtype, n, 1)
    g, _, _ = carried(B, dtype, n, 1)
    with f, g:
        res, H, var, _ = dense(st0, dtype, n, 2)
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


# ---- 12. refusals ---------------------------------------------------------------------------------------------------------------------------------

def test_refused_calls_launch_nothing():
    n = 18
    f, st0, _ = carried(B, 32, n, 1)
    with f:
        res, H, var, _ = dense(st0, 32, n, 3)
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


# ---- 13. re-acquisition ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,n,form", [(32, 18, "a"), (64, 15, "b")])
def test_position_fix_rows_against_a_grown_prior(dtype, n, form):
    """rows.position_fix (m = 3) against the prior grown by s = 1, 10, 100, judged as tests/test_reacquisition_gpu.py judges the velocity
    update: fp32 records by its rule (a), fp64 by (b), the state by (e).  (tests/test_rows_cpu.py checks that the rounded fp64 reference
    stays inside the domain of rule (a) on these inputs.)"""
    what = f"position_fix f{dtype} N={n}"
    f, st0, _ = carried(B, dtype, n, 0)
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
