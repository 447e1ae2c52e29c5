"""GPU suite of the body-velocity (DVL) update (include/fbus_ekf.h, fbus_ekf_correct_velocity*; csrc/ekf_velocity.hpp) against
tests/velocity_ref.py, the fp64 restatement on ekf_oracle_np.State: parity of one update and of a chain, NIS / gate / untouched lanes, the
five forms and a captured graph, per-filter variance, the likelihood sums, independence of the neighbours, and the refusals.
B = 193 (three 64-filter tiles and a tile of one) unless stated.

Why the fp32 kernel does its covariance arithmetic in double (measured on an MI355X).  support.state_batch behind three predicts carries a
prior velocity variance of 0.12 .. 0.18 (m/s)^2 -- the gravity prior of 100 reaches v through the predicts -- and the update takes it to
the order of var, 2.5e-5 .. 4e-4: a factor of 500 .. 2000 in one step.  With P - u u' / s in fp32 the block-wise covariance figure of
these cases came out at 1.9e-5 .. 3.45e-4 against COV_BLOCK_TOL = 1e-5, and diag(H P+ H') / var at 1.0008 after the chain's first update
(exact: 1 - 1e-3); a numpy emulation of the sequential and of the joint form in fp32 gave the same 4.0e-4.  With the joint form in double
and one rounding per element the same cases read 5.8e-8 .. 1.6e-7."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import depth_ref
import oracle_capi as oc
import velocity_ref as V
from fbus_ekf import BatchedFilter, capi, synth
from support import (B_IND, DT, imu_of, markers_of, permutation, poison_set, poisoned_state, r32, ragged_cut, same_rows, same_state,
                     state_batch, to_device)
from util import assert_parity, assert_window_parity

pytestmark = pytest.mark.gpu

B = B_IND
MOUNT = V.tilted_mount()                             # no zero entry
LEVER = np.array([0.21, -0.08, 0.12])
VAR = np.array([1e-4, 4e-4, 2.5e-5])
NAMES = ("nominal", "rot", "P", "prev")
NIS_TOL = {32: 1e-4, 64: 1e-9}                       # the depth suite's: in fp32 S inherits the covariance gate
FULL, BARE = (MOUNT, LEVER, True), (None, None, False)          # (mount, lever, gyro given)


def rnd(a, dtype):
    return r32(a) if dtype == 32 else np.asarray(a, np.float64)


def rel(a, b):
    return np.abs(a - b) / np.abs(b)


def ref_update(st, n, z, var, gyro, mount=MOUNT, lever=LEVER, thr3=np.inf, skip=None, joseph=False):
    """velocity_ref on every filter of get_state() arrays -> (state arrays, applied, nis, dof, ln det S)"""
    ss = V.states_of(st, n)
    var = np.broadcast_to(np.asarray(var, np.float64), (len(ss), 3))
    out = [V.correct_velocity(s, n, z[b], var[b], None if gyro is None else gyro[b], mount, lever, thr3,
                              bool(skip[b]) if skip is not None else False, joseph) for b, s in enumerate(ss)]
    app, nis, dof, lnd = (np.array(c) for c in zip(*out))
    return V.arrays_of(ss), app, nis, dof.astype(np.int32), lnd


def carried(nB, dtype, n, dialect, mount=MOUNT, lever=LEVER, seed_off=0):
    """a handle whose records hold a state of support.state_batch behind three predicts (the carried rotation is the stale one), its
    sensor set; returns (handle, its state as get_state() gives it, the rate sample that goes with the reading)"""
    prm, nom, rot, P, prev = state_batch(nB, dialect, n, seed_off=seed_off)
    f = BatchedFilter(nB, prm, device=0, dtype=dtype, nstate=n)
    f.set_state(nom, rot, P, prev)
    a, w = imu_of(seed_off, seed_off + nB, 0, 4, nom)
    for k in range(3):
        f.predict(a[k], w[k], DT)
    f.set_velocity_sensor(mount, lever)
    return f, f.get_state(), w[3]


def predicted(st, gyro, mount, lever):
    """h of the handle's own state, (B, 3) in double"""
    nom, rot = np.asarray(st[0], np.float64), np.asarray(st[1], np.float64).reshape(-1, 3, 3)
    y = np.einsum("bji,bj->bi", rot, nom[:, 3:6])
    if gyro is not None:
        y = y + np.cross(gyro - nom[:, 13:16], V.lever_of(lever))
    return y @ V.mount_of(mount).T


def readings(st, dtype, gyro, mount=MOUNT, lever=LEVER, seed=5):
    """z = h(the handle's own state) + N(0, diag(VAR)), representable in the record type"""
    e = np.random.default_rng(seed).normal(0, 1, (len(st[0]), 3)) * np.sqrt(VAR)
    return rnd(predicted(st, gyro, mount, lever) + e, dtype)


# ---- parity ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,n,dialect", [(d, n, dl) for d in (32, 64) for n in (18, 15) for dl in (0, 1)])
def test_one_update_against_the_restatement(dtype, n, dialect):
    for mount, lever, with_gyro in (FULL, BARE):
        f, st0, w = carried(B, dtype, n, dialect, mount, lever)
        gyro = w if with_gyro else None
        with f:
            # H_theta = C [R' v]x is in play on every filter
            Rtv = np.einsum("bji,bj->bi", np.asarray(st0[1], np.float64).reshape(-1, 3, 3), np.asarray(st0[0], np.float64)[:, 3:6])
            assert np.linalg.norm(Rtv, axis=1).min() > 1e-3
            z = readings(st0, dtype, gyro, mount, lever)
            nis, dof = f.correct_velocity_nis(z, VAR, gyro)
            got, app = f.get_state(), f.applied()
        assert app.all() and (dof == 3).all()
        for joseph in (False, True):
            ref, rapp, rnis, rdof, _ = ref_update(st0, n, z, VAR, gyro, mount, lever, joseph=joseph)
            assert rapp.all()
            print(f"nis rel err {rel(nis.astype(np.float64), rnis).max():.3e}")
            assert_parity(got, ref, dtype, f"correct_velocity f{dtype} N={n} dialect {dialect} full {with_gyro} joseph {joseph}")
            assert rel(nis.astype(np.float64), rnis).max() <= NIS_TOL[dtype]
        assert np.array_equal(got[1], st0[1]) and np.array_equal(got[3], st0[3])          # R and prev_id are not written
        if n == 15:
            assert np.array_equal(got[0][:, 16:19], st0[0][:, 16:19])                      # no gravity state: g stays
        if not with_gyro:
            # the gyro bias is not a column of H: it moves through its cross-covariance with v and theta alone (and it does move)
            assert not np.array_equal(got[0][:, 13:16], st0[0][:, 13:16])
            # ... and a lever without a rate sample is not used: the same bits as the sensor without one
            f, st1, _ = carried(B, dtype, n, dialect, mount, LEVER)
            with f:
                assert same_state(st0, st1)
                f.correct_velocity(z, VAR)
                assert same_state(got, f.get_state())


@pytest.mark.parametrize("nB", [1, 64])
def test_one_filter_and_one_full_tile(nB):
    f, st0, w = carried(nB, 32, 18, 1)
    with f:
        z = readings(st0, 32, w)
        f.correct_velocity(z, VAR, w)
        got = f.get_state()
        assert f.applied().all()
    assert_parity(got, ref_update(st0, 18, z, VAR, w)[0], 32, f"correct_velocity B = {nB}")


@pytest.mark.parametrize("n,dialect", [(18, 1), (15, 0)])
def test_a_chain_of_predicts_velocity_depth_and_pose_updates(n, dialect):
    """12 x (predict_n K = 7, correct_velocity), a stacked pose update every fourth step and a depth update every third, free-running
    against the oracle + depth_ref + velocity_ref"""
    K, STEPS = 7, 12
    AXIS, OFFSET, DLEVER, DVAR = np.array([0.12, -0.2, 1.0]), 0.4, np.array([0.11, -0.07, 0.05]), 1e-4
    prm, nom, rot, P, prev = state_batch(B, dialect, n)
    orc = oc.Oracle(dialect, n)
    ref = [np.array(nom), np.array(rot), np.array(P), np.array(prev)]
    Cm = V.mount_of(MOUNT)
    worst = []
    with BatchedFilter(B, prm, device=0, dtype=32, nstate=n) as f:
        f.set_state(nom, rot, P, prev)
        f.set_velocity_sensor(MOUNT, LEVER)
        f.set_depth_sensor(AXIS, OFFSET, DLEVER)
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
                zd = r32(synth.depth(0, B, step, nom, rot, axis=AXIS, offset=OFFSET, lever=DLEVER, noise=0.01))
                f.correct_depth(zd, DVAR)
                ss = V.states_of(ref, n)
                for b, s in enumerate(ss):
                    assert depth_ref.correct_depth(s, n, float(zd[b]), DVAR, AXIS, OFFSET, DLEVER)[0]
                ref = list(V.arrays_of(ss))
            w = gyr[K - 1]
            z = r32(synth.velocity(0, B, step, nom, rot, w, mount=MOUNT, lever=LEVER, noise=0.01))
            before = f.get_state()
            f.correct_velocity(z, VAR, w)
            after = f.get_state()
            assert f.applied().all()
            ref = list(ref_update(ref, n, z, VAR, w)[0])
            # the update shrinks the variance along its own rows: diag(H P+ H') < var (H P+ H' = R - R S^-1 R for the joint update), and
            # the velocity block does not grow
            R0, nom0 = np.asarray(before[1], np.float64).reshape(B, 3, 3), np.asarray(before[0], np.float64)
            H = np.zeros((B, 3, n))
            H[:, :, 3:6] = np.einsum("km,bjm->bkj", Cm, R0)
            wv = np.einsum("bji,bj->bi", R0, nom0[:, 3:6])
            H[:, :, 6:9] = np.einsum("km,bmj->bkj", Cm, np.array([depth_skew(x) for x in wv]))
            H[:, :, 12:15] = Cm @ depth_skew(LEVER)
            hph = np.einsum("bki,bij,bkj->bk", H, np.asarray(after[2], np.float64), H)
            tr = [np.trace(np.asarray(st[2], np.float64)[:, 3:6, 3:6], axis1=1, axis2=2) for st in (before, after)]
            worst.append(((hph / VAR).max(), (tr[1] / tr[0]).max()))
        got = f.get_state()
    for step, (rows, trace) in enumerate(worst):
        print(f"step {step}: max diag(H P+ H') / var = {rows:.6f}, max trace P_vv after / before = {trace:.6f}")
    try:
        assert_window_parity(got, ref, f"velocity chain N={n} dialect {dialect}", dialect, n)
    finally:
        for step, (rows, trace) in enumerate(worst):
            assert rows < 1.0, (step, rows)
            assert trace <= 1 + 1e-4, (step, trace)


def depth_skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


# ---- NIS, gate, untouched lanes -------------------------------------------------------------------------------------------------------------

def mixed_inputs(st0, dtype, w):
    """readings with a tail of outliers on one component, three distinct variance triples, and the lanes that must stay untouched.  Returns
    (z, gyro, var, skip, kinds): kinds[b] = 0 usable, 1 skipped, 2 NaN in a component of z, 3 a variance <= 0, 4 a NaN variance, 5 NaN in a
    component of gyro.  The lanes b % 32 == 19 are among the skipped ones (19 % 16 == 3) and carry a NaN rate as well; the rate rule has
    lanes of its own at b % 32 == 21: 12 + 12 + 6 + 6 + 6 = 42 of the 193 lanes are unusable."""
    nB = len(st0[0])
    b = np.arange(nB)
    z = np.array(readings(st0, dtype, w))
    z[b % 5 == 2, 1] += 2.0                                # outliers for the gate: S is of the order of the prior's 0.13 (m/s)^2
    z = rnd(z, dtype)
    var = (VAR[None, :] * np.array([1.0, 4.0, 0.25])[b % 3][:, None]).copy()
    gyro = np.array(w)
    kinds = np.zeros(nB, int)
    kinds[b % 16 == 3], kinds[b % 16 == 7], kinds[b % 32 == 11], kinds[b % 32 == 27], kinds[b % 32 == 21] = 1, 2, 3, 4, 5
    skip = (kinds == 1).astype(np.uint8)
    z[kinds == 2, b[kinds == 2] % 3] = np.nan
    var[kinds == 3, b[kinds == 3] % 3] = np.where(b[kinds == 3] % 64 == 11, 0.0, -1e-4)
    var[kinds == 4, b[kinds == 4] % 3] = np.nan
    gyro[(kinds == 5) | (b % 32 == 19), 2] = np.nan
    return z, gyro, var, skip, kinds


def gate_between(nis, share=0.9):
    """a threshold strictly between two neighbouring values of the sorted finite nis"""
    v = np.sort(nis[np.isfinite(nis) & (nis > 0)].astype(np.float64))
    i = int(share * len(v))
    assert v[i - 1] < v[i]
    return 0.5 * (v[i - 1] + v[i])


@pytest.mark.parametrize("dtype", [32, 64])
def test_nis_gate_and_untouched_lanes(dtype):
    n, dialect = 18, 1
    f, st0, w = carried(B, dtype, n, dialect)
    with f:
        z, gyro, var, skip, kinds = mixed_inputs(st0, dtype, w)
        nis0, _ = f.correct_velocity_nis(z, var, gyro, skip)          # ungated: the device's own nis
    thr3 = gate_between(nis0)
    f, st1, _ = carried(B, dtype, n, dialect)
    with f:
        assert same_state(st0, st1)
        f.set_gate([np.inf, np.inf, np.inf, thr3])
        nis, dof = f.correct_velocity_nis(z, var, gyro, skip)
        got, app = f.get_state(), f.applied()
    assert np.array_equal(nis, nis0)
    usable = kinds == 0
    assert (~usable).sum() == 42
    rejected = usable & ~(nis.astype(np.float64) <= thr3)
    applied = usable & ~rejected
    assert rejected.sum() >= 10 and np.array_equal(app.astype(bool), applied)
    assert (~applied).mean() <= 1 / 3, (~applied).mean()             # the applied-lane parity below is not vacuous
    assert np.array_equal(dof, 3 * usable.astype(np.int32))          # rejected 3; every unusable kind 0
    assert (nis[~usable] == 0).all() and all((kinds == k).sum() >= 6 for k in (1, 2, 3, 4, 5))
    assert same_state(st0, got, rows=np.nonzero(~applied)[0])       # record bytes unchanged
    # the restatement, ungated (the gate's decision is the device's, from its own nis): nis of every usable lane, the state of the applied
    ref, rapp, rnis, rdof, _ = ref_update(st0, n, z, var, gyro, skip=skip)
    assert np.array_equal(rapp, usable) and np.array_equal(rdof, dof)
    print(f"nis rel err {rel(nis.astype(np.float64)[usable], rnis[usable]).max():.3e}")
    assert rel(nis.astype(np.float64)[usable], rnis[usable]).max() <= NIS_TOL[dtype]
    sel = np.nonzero(applied)[0]
    assert_parity([x[sel] for x in got], [x[sel] for x in ref], dtype, f"gated correct_velocity f{dtype}: the applied lanes")


# ---- forms ------------------------------------------------------------------------------------------------------------------------------------

THR3 = 7.81                                          # chi-square, 3 degrees of freedom, 95 %: the outlier tail lies above it


def test_every_form_and_a_captured_graph_hold_the_same_bits():
    dtype, n, dialect = 32, 18, 1
    outs = {}
    z = None
    for form in ("host", "dev", "async", "nis null", "nis", "graph"):
        f, st0, w = carried(B, dtype, n, dialect)
        with f:
            if z is None:
                z, gyro, var, skip, _ = mixed_inputs(st0, dtype, w)
                z, gyro = z.astype(np.float32), gyro.astype(np.float32)
            f.set_gate([np.inf, np.inf, np.inf, THR3])
            dz, dg, dv, ds = to_device(z), to_device(gyro), to_device(var), to_device(skip)
            if form == "host":
                f.correct_velocity(z, var, gyro, skip)
            elif form == "dev":
                f.correct_velocity(dz, dv, dg, ds)
            elif form == "async":
                pin = lambda x: torch.from_numpy(np.ascontiguousarray(x)).pin_memory()
                f.correct_velocity_async(pin(z), pin(var), pin(gyro), pin(skip))
                f.async_inputs_consumed()
            elif form == "nis null":
                vp = lambda t: C.c_void_p(t.data_ptr())
                rc = f._lib.fbus_ekf_correct_velocity_nis_dev(f._h, vp(dz), vp(dg), vp(dv), 1, vp(ds), None, None)
                assert rc == 0
            elif form == "nis":
                f.correct_velocity_nis(dz, dv, dg, ds)
            else:
                gid = f.graph_capture(lambda: f.correct_velocity(dz, dv, dg, ds))
                f.sync()
                assert same_state(st0, f.get_state())                  # capturing launched nothing
                f.graph_launch(gid)
            f.sync()
            outs[form] = dict(zip(NAMES, f.get_state()), applied=f.applied())
    assert 0 < outs["host"]["applied"].sum() < B
    for form in outs:
        assert same_rows(outs["host"], outs[form]), form


def test_a_per_filter_variance_is_the_scalar_triple_of_a_handle_of_its_own():
    dtype, n, dialect = 32, 18, 0
    vals = VAR[None, :] * np.array([1.0, 4.0, 0.25])[:, None]
    f, st0, w = carried(B, dtype, n, dialect)
    with f:
        z = readings(st0, dtype, w)
        var = vals[np.arange(B) % 3]
        f.correct_velocity(z, var, w)
        whole = dict(zip(NAMES, f.get_state()), applied=f.applied())
    for k in range(3):
        f, _, _ = carried(B, dtype, n, dialect)
        with f:
            f.correct_velocity(z, vals[k], w)
            one = dict(zip(NAMES, f.get_state()), applied=f.applied())
        rows = np.nonzero(np.arange(B) % 3 == k)[0]
        assert same_rows(whole, one, rows, rows), k
    assert not same_rows(whole, one, np.arange(0, B, 3), np.arange(0, B, 3))      # (the variance does matter: rows of triple 0 under triple 2)


# ---- likelihood -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [32, 64])
def test_the_likelihood_sums(dtype):
    n, dialect = 18, 1
    res = {}
    for lik in (False, True):
        f, st0, w = carried(B, dtype, n, dialect)
        with f:
            z, gyro, var, skip, kinds = mixed_inputs(st0, dtype, w)
            f.set_gate([np.inf, np.inf, np.inf, THR3])
            if lik:
                f.loglik_enable()
                assert all((x == 0).all() for x in f.loglik())
            nis, dof = f.correct_velocity_nis(z, var, gyro, skip)
            res[lik] = dict(zip(NAMES, f.get_state()), applied=f.applied(), nis=nis, dof=dof)
            if lik:
                ll, rows, napp, nrej = f.loglik()
    assert same_rows(res[False], res[True])                          # the sums change no record, flag or output
    app = res[True]["applied"].astype(bool)
    rej = (kinds == 0) & ~app
    assert app.sum() > B // 2 and rej.sum() >= 10
    assert np.array_equal(rows, 3 * app.astype(np.int64)) and np.array_equal(napp, app.astype(np.int32))
    assert np.array_equal(nrej, rej.astype(np.int32))
    lnd = ref_update(st0, n, z, var, gyro, thr3=THR3, skip=skip)[4]
    want = -0.5 * (nis.astype(np.float64)[app] + lnd[app] + 3 * math.log(2 * math.pi))
    err = np.abs(ll[app] - want).max()
    print(f"f{dtype}: max |ll - (-1/2)(nis + ln det S + 3 ln 2 pi)| = {err:.3e}")
    assert err <= 1e-9 + NIS_TOL[dtype]
    assert (ll[~app] == 0).all() and (rows[~app] == 0).all()
    assert (nrej[kinds != 0] == 0).all() and (napp[kinds != 0] == 0).all()          # untouched lanes: no sum moves


# ---- independence ---------------------------------------------------------------------------------------------------------------------------------

def _job(dtype=32, n=18, dialect=1):
    f, st0, w = carried(B, dtype, n, dialect)
    f.close()
    z, gyro, var, skip, kinds = mixed_inputs(st0, dtype, w)
    ft = np.float32 if dtype == 32 else np.float64
    return st0, z.astype(ft), gyro.astype(ft), var, skip


def _run(st, z, gyro, var, skip, dtype=32, n=18, dialect=1, dev=False):
    """one gated update on a fresh handle holding exactly the state st; also returns the records as they were before it"""
    nB = len(st[0])
    prm = capi.default_params(dialect)
    dv = (lambda x: to_device(x)) if dev else (lambda x: x)
    with BatchedFilter(nB, prm, device=0, dtype=dtype, nstate=n) as f:
        f.set_state(*st)
        before = dict(zip(NAMES, f.get_state()))
        f.set_velocity_sensor(MOUNT, LEVER)
        f.set_gate([np.inf, np.inf, np.inf, THR3])
        nis, dof = f.correct_velocity_nis(dv(z), dv(var), dv(gyro), dv(skip))
        f.sync()
        if dev:
            nis, dof = nis.cpu().numpy(), dof.cpu().numpy()
        return dict(zip(NAMES, f.get_state()), applied=f.applied(), nis=nis, dof=dof), before


def test_a_filter_is_itself_wherever_it_stands():
    st0, z, gyro, var, skip = _job()
    v0, _ = _run(st0, z, gyro, var, skip)
    assert 0 < v0["applied"].sum() < B
    pi = permutation()
    assert same_rows(v0, _run([x[pi] for x in st0], z[pi], gyro[pi], var[pi], skip[pi])[0], rows=pi)
    # two handles cut inside a tile; the second reads SLICES of the whole job's device arrays, off the 16-byte boundary
    dz, dg, dv, ds = to_device(z), to_device(gyro), to_device(var), to_device(skip)
    for part in ragged_cut():
        lo, hi = part[0], part[-1] + 1
        if lo:
            assert dz[lo:hi].data_ptr() % 16 != 0 and dv[lo:hi].data_ptr() % 16 != 0
        assert same_rows(v0, _run([x[part] for x in st0], dz[lo:hi], dg[lo:hi], dv[lo:hi], ds[lo:hi], dev=True)[0], rows=part)


def test_a_clean_lane_among_broken_records_keeps_its_bits():
    st0, z, gyro, var, skip = _job()
    v0, _ = _run(st0, z, gyro, var, skip)
    S, form = poison_set()
    nom, rot, P = poisoned_state(st0[0], st0[1], st0[2], S, form)
    zz = z.copy()
    zz[S[form == 3], 0] = np.nan                                     # form (d): the input is broken, not the record
    out, before = _run([nom.astype(np.float32), rot.astype(np.float32), P.astype(np.float32), st0[3]], zz, gyro, var, skip)
    clean = np.setdiff1d(np.arange(B), S)
    assert 100 in clean and len(np.intersect1d(clean, np.arange(64, 128))) == 1          # a whole wave but one lane
    assert same_rows(v0, out, clean, clean)
    # A record of NaN (a: nis is NaN), one with a negated covariance (c: no positive pivot) and a broken reading (d) are not applied.
    # An infinite position with variances of 1e30 (b) and a zero rotation (e) leave S finite with positive pivots: the header's rule
    # -- pivots > 0 and nis <= thr[3] -- decides those, lane by lane.  Whatever is not applied keeps its bytes.
    usable = skip == 0
    usable[np.isnan(gyro).any(axis=1) | np.isnan(z).any(axis=1) | ~(var > 0).all(axis=1)] = False
    for k in (0, 2, 3):
        assert (out["applied"][S[form == k]] == 0).all(), k
    assert (out["dof"][S[(form == 0) | (form == 2)]] == 3 * usable[S[(form == 0) | (form == 2)]]).all()
    kept = S[out["applied"][S] == 0]
    assert len(kept) >= len(S) * 3 // 5
    assert same_rows(before, {k: out[k] for k in NAMES}, kept, kept)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------

def test_refused_calls_launch_nothing():
    prm, nom, rot, P, prev = state_batch(B, 1, 18)
    with BatchedFilter(B, prm, device=0, dtype=32, nstate=18) as f:
        f.set_state(nom, rot, P, prev)
        st0 = f.get_state()
        z, var = np.zeros((B, 3), np.float32), np.tile(VAR, (B, 1))
        dz, dv = to_device(z), to_device(var)
        last = lambda: f._lib.fbus_ekf_last_error(f._h).decode()
        for name, call in (("fbus_ekf_correct_velocity", lambda: f.correct_velocity(z, VAR)),
                           ("fbus_ekf_correct_velocity_dev", lambda: f.correct_velocity(dz, dv)),
                           ("fbus_ekf_correct_velocity_async", lambda: f.correct_velocity_async(z, VAR)),
                           ("fbus_ekf_correct_velocity_nis", lambda: f.correct_velocity_nis(z, VAR)),
                           ("fbus_ekf_correct_velocity_nis_dev", lambda: f.correct_velocity_nis(dz, dv))):
            with pytest.raises(capi.FbusError) as e:                 # before set_velocity_sensor
                call()
            assert e.value.code == 1 and "fbus_ekf_set_velocity_sensor" in str(e.value) and name + ":" in str(e.value), str(e.value)
        skewed, nan_mount = MOUNT.copy(), MOUNT.copy()
        skewed[0, 1] += 1e-3                                          # max |C C' - I| ~ 1e-3
        nan_mount[2, 2] = np.nan
        for mount, lever in ((skewed, None), (2.0 * np.eye(3), None), (nan_mount, None), (np.full((3, 3), np.inf), None),
                             (MOUNT, [0.0, np.nan, 0.0])):
            with pytest.raises(capi.FbusError) as e:
                f.set_velocity_sensor(mount, lever)
            assert e.value.code == 1 and "fbus_ekf_set_velocity_sensor" in str(e.value)
        with pytest.raises(capi.FbusError):                           # (a refused setter sets nothing)
            f.correct_velocity(z, VAR)
        f.set_velocity_sensor(MOUNT, LEVER)
        vp = lambda t: C.c_void_p(t.data_ptr())
        for name in ("fbus_ekf_correct_velocity_dev", "fbus_ekf_correct_velocity_nis_dev"):
            tail = (None, None) if "nis" in name else ()
            assert getattr(f._lib, name)(f._h, vp(dz), None, vp(dv), 2, None, *tail) == 1
            assert name in last() and "var_per_filter" in last()
            assert getattr(f._lib, name)(f._h, None, None, vp(dv), 0, None, *tail) == 1
            assert name in last()
            assert getattr(f._lib, name)(f._h, vp(dz), None, None, 0, None, *tail) == 1
            assert name in last()
        # inside a capture: the setter and the host form
        f._check(f._lib.fbus_ekf_graph_begin(f._h), "graph_begin")
        try:
            mt = (C.c_double * 9)(*np.eye(3).ravel())
            assert f._lib.fbus_ekf_set_velocity_sensor(f._h, mt, None) == 1
            assert "fbus_ekf_set_velocity_sensor" in last()
            hz, hv = z.ctypes.data_as(C.c_void_p), var.ctypes.data_as(C.c_void_p)
            assert f._lib.fbus_ekf_correct_velocity(f._h, hz, None, hv, 1, None) == 1
            assert "fbus_ekf_correct_velocity:" in last()
            assert f._lib.fbus_ekf_correct_velocity_nis(f._h, hz, None, hv, 1, None, None, None) == 1
            assert "fbus_ekf_correct_velocity_nis:" in last()
        finally:
            gid = C.c_int(-1)
            f._lib.fbus_ekf_graph_end(f._h, C.byref(gid))
        f.sync()
        assert same_state(st0, f.get_state()) and (f.applied() == 0).all()
        # the refused setter inside the capture kept the sensor: the bits of a handle that was given the tilted mount and nothing else
        zr = readings(st0, 32, None, MOUNT, None)
        f.correct_velocity(zr, VAR)
        got = f.get_state()
    with BatchedFilter(B, prm, device=0, dtype=32, nstate=18) as f:
        f.set_state(nom, rot, P, prev)
        f.set_velocity_sensor(MOUNT, LEVER)
        f.correct_velocity(zr, VAR)
        assert same_state(got, f.get_state()) and not same_state(got, st0)
