"""GPU suite of the depth (pressure) sensor update (include/fbus_ekf.h, fbus_ekf_correct_depth*; csrc/ekf_depth.hpp) against
tests/depth_ref.py, the fp64 restatement on ekf_oracle_np.State: parity of one update and of a chain, NIS / gate / untouched lanes, the
five forms and a captured graph, per-filter variance, the likelihood sums, independence of the neighbours, and the refusals.
B = 193 (three 64-filter tiles and a tile of one) unless stated."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import depth_ref
import ekf_oracle_np as E
import oracle_capi as oc
from fbus_ekf import BatchedFilter, capi, synth
from support import (B_IND, DT, imu_of, markers_of, permutation, poison_set, poisoned_state, r32, ragged_cut, same_rows, same_state,
                     state_batch, to_device)
from util import assert_parity, assert_window_parity

pytestmark = pytest.mark.gpu

B = B_IND
AXIS = np.array([0.12, -0.2, 1.0])                   # tilted
LEVER = np.array([0.11, -0.07, 0.05])
OFFSET = 0.4
VAR = 1e-4                                           # a 1 cm sensor beside a prior of ~1 cm in position
NAMES = ("nominal", "rot", "P", "prev")


def rnd(a, dtype):
    return r32(a) if dtype == 32 else np.asarray(a, np.float64)


def states_of(st, n):
    """get_state() arrays -> one ekf_oracle_np.State per filter, in double"""
    nom, rot, P, prev = (np.asarray(x, np.float64) if i < 3 else np.asarray(x) for i, x in enumerate(st))
    out = []
    for b in range(len(nom)):
        s = E.State(n)
        s.p, s.v, s.q, s.ba, s.bg, s.g = (nom[b, a:e].copy() for a, e in ((0, 3), (3, 6), (6, 10), (10, 13), (13, 16), (16, 19)))
        s.R, s.P, s.prev_id = rot[b].reshape(3, 3).copy(), P[b].copy(), int(prev[b])
        out.append(s)
    return out


def arrays_of(states):
    nom = np.array([np.concatenate([s.p, s.v, s.q, s.ba, s.bg, s.g]) for s in states])
    return nom, np.array([s.R.ravel() for s in states]), np.array([s.P for s in states]), np.array([s.prev_id for s in states], np.int32)


def ref_update(st, n, z, var, lever=LEVER, thr1=np.inf, skip=None, joseph=False):
    """depth_ref on every filter of get_state() arrays -> (state arrays, applied, nis, dof, S)"""
    ss = states_of(st, n)
    var = np.broadcast_to(np.asarray(var, np.float64), (len(ss),))
    out = [depth_ref.correct_depth(s, n, float(z[b]), float(var[b]), AXIS, OFFSET, lever, thr1, bool(skip[b]) if skip is not None else False,
                                   joseph) for b, s in enumerate(ss)]
    app, nis, dof, S = (np.array(c) for c in zip(*out))
    return arrays_of(ss), app, nis, dof.astype(np.int32), S


def carried(nB, dtype, n, dialect, lever=LEVER, seed_off=0):
    """a handle whose records hold a state of support.state_batch behind three predicts (the carried rotation is the stale one), its
    sensor set; returns (handle, its state as get_state() gives it)"""
    prm, nom, rot, P, prev = state_batch(nB, dialect, n, seed_off=seed_off)
    f = BatchedFilter(nB, prm, device=0, dtype=dtype, nstate=n)
    f.set_state(nom, rot, P, prev)
    a, w = imu_of(seed_off, seed_off + nB, 0, 3, nom)
    for k in range(3):
        f.predict(a[k], w[k], DT)
    f.set_depth_sensor(AXIS, OFFSET, lever)
    return f, f.get_state()


def readings(st, dtype, lever=LEVER, seed=5, sigma=0.01):
    """z = h(the handle's own state) + N(0, sigma^2), representable in the record type"""
    nom, rot = np.asarray(st[0], np.float64), np.asarray(st[1], np.float64)
    lv = depth_ref.lever_of(lever)
    hx = (nom[:, 0:3] + rot.reshape(-1, 3, 3) @ lv) @ depth_ref.unit(AXIS) + OFFSET
    return rnd(hx + np.random.default_rng(seed).normal(0, sigma, len(nom)), dtype)


def rel(a, b):
    return np.abs(a - b) / np.abs(b)


NIS_TOL = {32: 1e-4, 64: 1e-9}                       # fp32: S inherits the covariance gate


# ---- parity ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,n,dialect", [(d, n, dl) for d in (32, 64) for n in (18, 15) for dl in (0, 1)])
def test_one_update_against_the_restatement(dtype, n, dialect):
    for lever in (LEVER, None):
        f, st0 = carried(B, dtype, n, dialect, lever)
        with f:
            z = readings(st0, dtype, lever)
            nis, dof = f.correct_depth_nis(z, VAR)
            got, app = f.get_state(), f.applied()
        assert app.all() and (dof == 1).all()
        for joseph in (False, True):
            ref, rapp, rnis, rdof, _ = ref_update(st0, n, z, VAR, lever, joseph=joseph)
            assert rapp.all()
            assert_parity(got, ref, dtype, f"correct_depth f{dtype} N={n} dialect {dialect} lever {lever is not None} joseph {joseph}")
            assert rel(nis.astype(np.float64), rnis).max() <= NIS_TOL[dtype]
        assert np.array_equal(got[1], st0[1]) and np.array_equal(got[3], st0[3])          # R and prev_id are not written
        if n == 15:
            assert np.array_equal(got[0][:, 16:19], st0[0][:, 16:19])                      # no gravity state: g stays


@pytest.mark.parametrize("nB", [1, 64])
def test_one_filter_and_one_full_tile(nB):
    f, st0 = carried(nB, 32, 18, 1)
    with f:
        z = readings(st0, 32)
        f.correct_depth(z, VAR)
        got = f.get_state()
        assert f.applied().all()
    assert_parity(got, ref_update(st0, 18, z, VAR)[0], 32, f"correct_depth B = {nB}")


@pytest.mark.parametrize("n,dialect", [(18, 1), (15, 0)])
def test_a_chain_of_predicts_depth_updates_and_pose_updates(n, dialect):
    """12 x (predict_n K = 7, correct_depth), a stacked pose update every fourth step, free-running against the oracle + depth_ref"""
    K, STEPS = 7, 12
    prm, nom, rot, P, prev = state_batch(B, dialect, n)
    a_unit = depth_ref.unit(AXIS)
    orc = oc.Oracle(dialect, n)
    ref = [np.array(nom), np.array(rot), np.array(P), np.array(prev)]
    with BatchedFilter(B, prm, device=0, dtype=32, nstate=n) as f:
        f.set_state(nom, rot, P, prev)
        f.set_depth_sensor(AXIS, OFFSET, LEVER)
        for step in range(STEPS):
            acc, gyr = imu_of(0, B, step * K, K, nom)
            f.predict_n(acc, gyr, np.repeat(DT, K))
            for k in range(K):
                orc.predict(*ref, acc[k], gyr[k], DT)
            if step % 4 == 3:
                ids, pos, quat = markers_of(0, B, step, 4, nom, prm)
                f.correct(ids, pos, quat, capi.MODE_STACKED)
                orc.correct(*ref, ids, pos, quat, oc.STACKED)
            z = r32(synth.depth(0, B, step, nom, rot, axis=AXIS, offset=OFFSET, lever=LEVER, noise=0.01))
            before = f.get_state()
            f.correct_depth(z, VAR)
            after = f.get_state()
            assert f.applied().all()
            ref = list(ref_update(ref, n, z, VAR)[0])
            # the update shrinks the variance along its own row: H P H' < var afterwards, and never above its value before
            hph = []
            for st in (before, after):
                R, Pm = np.asarray(st[1], np.float64).reshape(B, 3, 3), np.asarray(st[2], np.float64)
                H = np.zeros((B, n))
                H[:, 0:3] = a_unit
                H[:, 6:9] = np.cross(LEVER, np.einsum("bji,j->bi", R, a_unit))
                hph.append(np.einsum("bi,bij,bj->b", H, Pm, H))
            assert (hph[1] < VAR).all(), (step, hph[1].max())
            assert (hph[1] <= hph[0] * (1 + 1e-4)).all(), step
        got = f.get_state()
    assert_window_parity(got, ref, f"depth chain N={n} dialect {dialect}", dialect, n)


# ---- NIS, gate, untouched lanes -------------------------------------------------------------------------------------------------------------

def mixed_inputs(st0, dtype):
    """readings with a tail of outliers, three distinct variances, and the lanes that must stay untouched.  Returns (z, var, skip, kinds):
    kinds[b] = 0 usable, 1 skipped, 2 NaN z, 3 var <= 0, 4 NaN var"""
    nB = len(st0[0])
    b = np.arange(nB)
    z = np.array(readings(st0, dtype))
    z[b % 5 == 2] += 0.08                                  # outliers for the gate
    z = rnd(z, dtype)
    var = np.array([1e-4, 4e-4, 2.5e-5])[b % 3].copy()
    kinds = np.zeros(nB, int)
    kinds[b % 16 == 3], kinds[b % 16 == 7], kinds[b % 32 == 11], kinds[b % 32 == 27] = 1, 2, 3, 4
    skip = (kinds == 1).astype(np.uint8)
    z[kinds == 2] = np.nan
    var[kinds == 3] = np.where(b[kinds == 3] % 64 == 11, 0.0, -1e-4)
    var[kinds == 4] = np.nan
    return z, var, skip, kinds


def gate_between(nis, share=0.85):
    """a threshold strictly between two neighbouring values of the sorted finite nis"""
    v = np.sort(nis[np.isfinite(nis) & (nis > 0)].astype(np.float64))
    i = int(share * len(v))
    assert v[i - 1] < v[i]
    return 0.5 * (v[i - 1] + v[i])


@pytest.mark.parametrize("dtype", [32, 64])
def test_nis_gate_and_untouched_lanes(dtype):
    n, dialect = 18, 1
    f, st0 = carried(B, dtype, n, dialect)
    with f:
        z, var, skip, kinds = mixed_inputs(st0, dtype)
        nis0, _ = f.correct_depth_nis(z, var, skip)                  # ungated: the device's own nis
    thr1 = gate_between(nis0)
    f, st1 = carried(B, dtype, n, dialect)
    with f:
        assert same_state(st0, st1)
        f.set_gate([np.inf, thr1])
        nis, dof = f.correct_depth_nis(z, var, skip)
        got, app = f.get_state(), f.applied()
    assert np.array_equal(nis, nis0)
    usable = kinds == 0
    rejected = usable & (nis.astype(np.float64) > thr1)
    applied = usable & ~rejected
    assert rejected.sum() >= 10 and np.array_equal(app.astype(bool), applied)
    assert (~applied).mean() <= 1 / 3, (~applied).mean()             # the applied-lane parity below is not vacuous
    assert np.array_equal(dof, usable.astype(np.int32))              # rejected 1; skipped, NaN z, var <= 0, NaN var 0
    assert (nis[~usable] == 0).all() and all((kinds == k).sum() >= 6 for k in (1, 2, 3, 4))
    assert same_state(st0, got, rows=np.nonzero(~applied)[0])       # record bytes unchanged
    # the restatement, ungated (the gate's decision is the device's, from its own nis): nis of every usable lane, the state of the applied
    ref, rapp, rnis, rdof, _ = ref_update(st0, n, z, var, skip=skip)
    assert np.array_equal(rapp, usable) and np.array_equal(rdof, dof)
    assert rel(nis.astype(np.float64)[usable], rnis[usable]).max() <= NIS_TOL[dtype]
    sel = np.nonzero(applied)[0]
    assert_parity([x[sel] for x in got], [x[sel] for x in ref], dtype, f"gated correct_depth f{dtype}: the applied lanes")


# ---- forms ------------------------------------------------------------------------------------------------------------------------------------

def test_every_form_and_a_captured_graph_hold_the_same_bits():
    dtype, n, dialect = 32, 18, 1
    outs = {}
    z = var = skip = thr1 = None
    for form in ("host", "dev", "async", "nis null", "nis", "graph"):
        f, st0 = carried(B, dtype, n, dialect)
        with f:
            if z is None:
                z, var, skip, _ = mixed_inputs(st0, dtype)
                z = z.astype(np.float32)
                thr1 = 4.0
            f.set_gate([np.inf, thr1])
            dz, dv, ds = to_device(z), to_device(var), to_device(skip)
            if form == "host":
                f.correct_depth(z, var, skip)
            elif form == "dev":
                f.correct_depth(dz, dv, ds)
            elif form == "async":
                pin = lambda x: torch.from_numpy(np.ascontiguousarray(x)).pin_memory()
                f.correct_depth_async(pin(z), pin(var), pin(skip))
                f.async_inputs_consumed()
            elif form == "nis null":
                rc = f._lib.fbus_ekf_correct_depth_nis_dev(f._h, C.c_void_p(dz.data_ptr()), C.c_void_p(dv.data_ptr()), 1,
                                                           C.c_void_p(ds.data_ptr()), None, None)
                assert rc == 0
            elif form == "nis":
                f.correct_depth_nis(dz, dv, ds)
            else:
                gid = f.graph_capture(lambda: f.correct_depth(dz, dv, ds))
                f.sync()
                assert same_state(st0, f.get_state())                  # capturing launched nothing
                f.graph_launch(gid)
            f.sync()
            outs[form] = dict(zip(NAMES, f.get_state()), applied=f.applied())
    assert 0 < outs["host"]["applied"].sum() < B
    for form in outs:
        assert same_rows(outs["host"], outs[form]), form


def test_a_per_filter_variance_is_the_scalar_of_a_handle_of_its_own():
    dtype, n, dialect = 32, 18, 0
    vals = np.array([1e-4, 4e-4, 2.5e-5])
    f, st0 = carried(B, dtype, n, dialect)
    with f:
        z = readings(st0, dtype)
        var = vals[np.arange(B) % 3]
        f.correct_depth(z, var)
        whole = dict(zip(NAMES, f.get_state()), applied=f.applied())
    for k in range(3):
        f, _ = carried(B, dtype, n, dialect)
        with f:
            f.correct_depth(z, float(vals[k]))
            one = dict(zip(NAMES, f.get_state()), applied=f.applied())
        rows = np.nonzero(np.arange(B) % 3 == k)[0]
        assert same_rows(whole, one, rows, rows), k
    assert not same_rows(whole, one, np.arange(0, B, 3), np.arange(0, B, 3))      # (the variance does matter: rows of var 0 under var 2)


# ---- likelihood -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [32, 64])
def test_the_likelihood_sums(dtype):
    n, dialect, thr1 = 18, 1, 4.0
    res = {}
    for lik in (False, True):
        f, st0 = carried(B, dtype, n, dialect)
        with f:
            z, var, skip, kinds = mixed_inputs(st0, dtype)
            f.set_gate([np.inf, thr1])
            if lik:
                f.loglik_enable()
                assert all((x == 0).all() for x in f.loglik())
            nis, dof = f.correct_depth_nis(z, var, skip)
            res[lik] = dict(zip(NAMES, f.get_state()), applied=f.applied(), nis=nis, dof=dof)
            if lik:
                ll, rows, napp, nrej = f.loglik()
    assert same_rows(res[False], res[True])                          # the sums change no record, flag or output
    app = res[True]["applied"].astype(bool)
    rej = (kinds == 0) & ~app
    assert app.sum() > B // 2 and rej.sum() >= 10
    assert np.array_equal(rows, app.astype(np.int64)) and np.array_equal(napp, app.astype(np.int32))
    assert np.array_equal(nrej, rej.astype(np.int32))
    S = ref_update(st0, n, z, var, thr1=thr1, skip=skip)[4]
    want = -0.5 * (nis.astype(np.float64)[app] + np.log(S[app]) + math.log(2 * math.pi))
    err = np.abs(ll[app] - want).max()
    print(f"f{dtype}: max |ll - (-1/2)(nis + ln S + ln 2 pi)| = {err:.3e}")
    assert err <= 1e-9 + NIS_TOL[dtype]
    assert (ll[~app] == 0).all()


# ---- independence ---------------------------------------------------------------------------------------------------------------------------------

def _job(dtype=32, n=18, dialect=1):
    f, st0 = carried(B, dtype, n, dialect)
    f.close()
    z, var, skip, kinds = mixed_inputs(st0, dtype)
    return st0, z.astype(np.float32 if dtype == 32 else np.float64), var, skip


def _run(st, z, var, skip, dtype=32, n=18, dialect=1, dev=False):
    """one gated update on a fresh handle holding exactly the state st"""
    nB = len(st[0])
    prm = capi.default_params(dialect)
    with BatchedFilter(nB, prm, device=0, dtype=dtype, nstate=n) as f:
        f.set_state(*st)
        f.set_depth_sensor(AXIS, OFFSET, LEVER)
        f.set_gate([np.inf, 4.0])
        nis, dof = f.correct_depth_nis(to_device(z) if dev else z, to_device(var) if dev else var, to_device(skip) if dev else skip)
        f.sync()
        if dev:
            nis, dof = nis.cpu().numpy(), dof.cpu().numpy()
        return dict(zip(NAMES, f.get_state()), applied=f.applied(), nis=nis, dof=dof)


def test_a_filter_is_itself_wherever_it_stands():
    st0, z, var, skip = _job()
    v0 = _run(st0, z, var, skip)
    assert 0 < v0["applied"].sum() < B
    pi = permutation()
    assert same_rows(v0, _run([x[pi] for x in st0], z[pi], var[pi], skip[pi]), rows=pi)
    # two handles cut inside a tile; the second reads SLICES of the whole job's device arrays, off the 16-byte boundary
    dz, dv, ds = to_device(z), to_device(var), to_device(skip)
    for part in ragged_cut():
        lo, hi = part[0], part[-1] + 1
        if lo:
            assert dz[lo:hi].data_ptr() % 16 != 0 and dv[lo:hi].data_ptr() % 16 != 0
        assert same_rows(v0, _run([x[part] for x in st0], dz[lo:hi], dv[lo:hi], ds[lo:hi], dev=True), rows=part)


def test_a_clean_lane_among_broken_records_keeps_its_bits():
    st0, z, var, skip = _job()
    v0 = _run(st0, z, var, skip)
    S, form = poison_set()
    nom, rot, P = poisoned_state(st0[0], st0[1], st0[2], S, form)
    zz = z.copy()
    zz[S[form == 3]] = np.nan                                        # form (d): the input is broken, not the record
    # form (c): the suite's variances (2.5e-5 .. 4e-4) straddle the prior's H P H' (0.85e-4 .. 1.4e-4), and a negated covariance under
    # var = 4e-4 leaves S > 0: a lane the rule applies.  Under the smallest of the three every negated covariance gives S < 0.
    vv = var.copy()
    vv[S[form == 2]] = 2.5e-5
    broken = [nom.astype(np.float32), rot.astype(np.float32), P.astype(np.float32), st0[3]]
    with BatchedFilter(B, capi.default_params(1), device=0, dtype=32, nstate=18) as f:
        f.set_state(*broken)
        before = dict(zip(NAMES, f.get_state()))                     # the records as they were before the update
    out = _run(broken, zz, vv, skip)
    clean = np.setdiff1d(np.arange(B), S)
    assert 100 in clean and len(np.intersect1d(clean, np.arange(64, 128))) == 1          # a whole wave but one lane
    assert same_rows(v0, out, clean, clean)
    # A record of NaN (a: nis is NaN), one with a negated covariance (c: S = H P H' + var < 0) and a broken reading (d) are not applied.
    # An infinite position with variances of 1e30 (b) and a zero rotation (e) leave S finite and positive: the header's rule -- S > 0 and
    # nis <= thr[1] -- decides those, lane by lane.  Whatever is not applied keeps its bytes.
    usable = (skip == 0) & np.isfinite(zz) & np.isfinite(vv) & (vv > 0)
    for k in (0, 2, 3):
        assert (out["applied"][S[form == k]] == 0).all(), k
    ac = S[(form == 0) | (form == 2)]
    assert (out["dof"][ac] == usable[ac]).all() and np.isnan(out["nis"][S[form == 0]][usable[S[form == 0]]]).all()
    kept = S[out["applied"][S] == 0]
    assert len(kept) >= len(S) * 3 // 5
    assert same_rows(before, {k: out[k] for k in NAMES}, kept, kept)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------

def test_refused_calls_launch_nothing():
    prm, nom, rot, P, prev = state_batch(B, 1, 18)
    with BatchedFilter(B, prm, device=0, dtype=32, nstate=18) as f:
        f.set_state(nom, rot, P, prev)
        st0 = f.get_state()
        z, var = np.zeros(B, np.float32), np.full(B, VAR)
        dz, dv = to_device(z), to_device(var)
        for name, call in (("fbus_ekf_correct_depth", lambda: f.correct_depth(z, VAR)),
                           ("fbus_ekf_correct_depth_dev", lambda: f.correct_depth(dz, dv)),
                           ("fbus_ekf_correct_depth_async", lambda: f.correct_depth_async(z, VAR)),
                           ("fbus_ekf_correct_depth_nis", lambda: f.correct_depth_nis(z, VAR)),
                           ("fbus_ekf_correct_depth_nis_dev", lambda: f.correct_depth_nis(dz, dv))):
            with pytest.raises(capi.FbusError) as e:                 # before set_depth_sensor
                call()
            assert e.value.code == 1 and "fbus_ekf_set_depth_sensor" in str(e.value) and name + ":" in str(e.value), str(e.value)
        for axis in ([0.0, 0.0, 0.0], [np.nan, 0.0, 1.0], [np.inf, 0.0, 0.0]):
            with pytest.raises(capi.FbusError) as e:
                f.set_depth_sensor(axis)
            assert e.value.code == 1 and "fbus_ekf_set_depth_sensor" in str(e.value)
        with pytest.raises(capi.FbusError):                           # (a refused setter sets nothing)
            f.correct_depth(z, VAR)
        f.set_depth_sensor(AXIS, OFFSET, LEVER)
        vp = lambda t: C.c_void_p(t.data_ptr())
        for name in ("fbus_ekf_correct_depth_dev", "fbus_ekf_correct_depth_nis_dev"):
            tail = (None, None) if "nis" in name else ()
            assert getattr(f._lib, name)(f._h, vp(dz), vp(dv), 2, None, *tail) == 1
            assert name in f._lib.fbus_ekf_last_error(f._h).decode() and "var_per_filter" in f._lib.fbus_ekf_last_error(f._h).decode()
            assert getattr(f._lib, name)(f._h, None, vp(dv), 0, None, *tail) == 1
            assert name in f._lib.fbus_ekf_last_error(f._h).decode()
        f.sync()
        assert same_state(st0, f.get_state()) and (f.applied() == 0).all()
