"""GPU suite that the three streamed sensor updates share (include/fbus_ekf.h, fbus_ekf_correct_depth* / _velocity* / _rows*; one copy of the
exits, the gate rule, the row steps and the passes in csrc/ekf_sensor.hpp), every test once and every family of tests/sensor_families.py
through it, against the fp64 restatements on ekf_oracle_np.State: parity of one filter and one full tile, NIS / gate / untouched lanes,
every form and a captured graph, per-filter variance, the likelihood sums, independence of the neighbours.  What is a family's own -- its
chain, its refusals -- is in tests/test_depth_gpu.py, test_velocity_gpu.py and test_rows_gpu.py, and so are the cases of the one-update
parity test, under the ids they have always had: its one body is sensor_families.one_update.
tests/test_sensor_suite_cpu.py holds the conditions that keep these tests from being vacuous.  B = 193 (three 64-filter tiles and a
tile of one); the states are support.state_batch behind three predicts, so the carried rotation is the stale one."""
import math

import numpy as np
import pytest

import sensor_families as F
from fbus_ekf import BatchedFilter, capi
from sensor_families import NAMES, NIS_TOL, gate_between, outs, rel
from support import B_IND, permutation, poison_set, poisoned_state, ragged_cut, same_rows, same_state, to_device
from util import assert_parity

pytestmark = pytest.mark.gpu

B = B_IND
FAMILIES = [pytest.param(F.Depth(), id="depth"), pytest.param(F.Velocity(), id="velocity"), pytest.param(F.Rows(3), id="rows")]


def on_device(inp):
    return {k: to_device(v) for k, v in inp.items()}


# ---- parity ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nB", [1, 64])
@pytest.mark.parametrize("fam", FAMILIES)
def test_one_filter_and_one_full_tile(fam, nB):
    f, st0, aux = fam.handle(nB, 32, 18, 1)
    with f:
        inp = fam.readings(st0, 32, aux)
        fam.call(f, inp, "host")
        got = f.get_state()
        assert f.applied().all()
    assert_parity(got, fam.ref(st0, 18, inp)[0], 32, f"{fam} B = {nB}")


# ---- NIS, gate, untouched lanes -------------------------------------------------------------------------------------------------------------

def missing_gate_entry_is_refused(fam, f, st0, inp):
    """a gate table of m entries has no thr[m]: both forms refuse and launch nothing"""
    f.set_gate([np.inf] * fam.rows)
    for call in (lambda: fam.call(f, inp, "host"), lambda: fam.call(f, on_device({k: inp[k] for k in fam.keys}), "nis dev")):
        with pytest.raises(capi.FbusError) as e:
            call()
        assert e.value.code == 1 and "fbus_ekf_correct_rows" in str(e.value) and "gate table" in str(e.value)
    f.sync()
    assert same_state(st0, f.get_state())


@pytest.mark.parametrize("dtype", [32, 64])
@pytest.mark.parametrize("fam", FAMILIES)
def test_nis_gate_and_untouched_lanes(fam, dtype):
    n, dialect = 18, 1
    f, st0, aux = fam.handle(B, dtype, n, dialect)
    with f:
        inp = fam.mixed(st0, dtype, aux)
        nis0, _ = fam.call(f, inp, "nis")                            # ungated: the device's own nis
    kinds = inp["kinds"]
    thr = gate_between(nis0, fam.SHARE)
    f, st1, _ = fam.handle(B, dtype, n, dialect)
    with f:
        assert same_state(st0, st1)
        if fam.name == "rows":
            missing_gate_entry_is_refused(fam, f, st0, inp)
        f.set_gate(fam.gate(thr))
        nis, dof = fam.call(f, inp, "nis")
        got, app = f.get_state(), f.applied()
    assert np.array_equal(nis, nis0)
    usable = kinds == 0
    assert (~usable).sum() == fam.UNUSABLE and all((kinds == k).sum() >= 6 for k in range(1, fam.KINDS + 1))
    rejected = usable & ~(nis.astype(np.float64) <= thr)
    applied = usable & ~rejected
    assert rejected.sum() >= 10 and np.array_equal(app.astype(bool), applied)
    assert (~applied).mean() <= fam.CAP, (~applied).mean()           # the applied-lane parity below is not vacuous
    assert np.array_equal(dof, fam.rows * usable.astype(np.int32))   # rejected: rows; every unusable kind 0
    assert (nis[~usable] == 0).all()
    assert same_state(st0, got, rows=np.nonzero(~applied)[0])       # record bytes unchanged
    # the restatement, ungated (the gate's decision is the device's, from its own nis): nis of every usable lane, the state of the applied
    ref, rapp, rnis, rdof, _ = fam.ref(st0, n, inp)
    assert np.array_equal(rapp, usable) and np.array_equal(rdof, dof)
    print(f"nis rel err {rel(nis.astype(np.float64)[usable], rnis[usable]).max():.3e}")
    assert rel(nis.astype(np.float64)[usable], rnis[usable]).max() <= NIS_TOL[dtype]
    sel = np.nonzero(applied)[0]
    assert_parity([x[sel] for x in got], [x[sel] for x in ref], dtype, f"gated {fam} f{dtype}: the applied lanes")


# ---- forms ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fam", FAMILIES)
def test_every_form_and_a_captured_graph_hold_the_same_bits(fam):
    dtype, n, dialect = 32, 18, 1
    got = {}
    inp = None
    for form in fam.FORMS:
        f, st0, aux = fam.handle(B, dtype, n, dialect)
        with f:
            if inp is None:
                inp = fam.cast(fam.mixed(st0, dtype, aux), dtype)
            f.set_gate(fam.gate(fam.THR))
            dev = on_device(inp)
            if form == "graph":
                gid = f.graph_capture(lambda: fam.call(f, dev, "dev"))
                f.sync()
                assert same_state(st0, f.get_state())                  # capturing launched nothing
                f.graph_launch(gid)
            else:
                fam.call(f, dev if form in fam.DEVICE_FORMS else inp, form)
            f.sync()
            got[form] = outs(f)
    assert 0 < got["host"]["applied"].sum() < B
    for form in got:
        assert same_rows(got["host"], got[form]), form


@pytest.mark.parametrize("fam", FAMILIES)
def test_a_per_filter_variance_is_the_scalar_set_of_a_handle_of_its_own(fam):
    dtype, n, dialect = 32, 18, 0
    f, st0, aux = fam.handle(B, dtype, n, dialect)
    with f:
        inp, groups = fam.per_filter(fam.readings(st0, dtype, aux))
        fam.call(f, inp, "host")
        whole = outs(f)
    for var, rows in groups:
        f, _, _ = fam.handle(B, dtype, n, dialect)
        with f:
            fam.call(f, dict(inp, var=var), "host")                  # the scalars of one group for every filter
            one = outs(f)
        assert same_rows(whole, one, rows, rows), rows[0]
    for _, other in groups[:-1]:
        assert not same_rows(whole, one, other, other)                # (the variance does matter: the other groups under the last one's)


# ---- likelihood -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [32, 64])
@pytest.mark.parametrize("fam", FAMILIES)
def test_the_likelihood_sums(fam, dtype):
    """one gated call with untouched lanes; where the family declares a SECOND call (rows: m = 1 on the new state, on every lane) the
    sums are those of both, against the restatement's ln det S"""
    n, dialect = 18, 1
    gate = fam.gate(fam.THR)
    two = fam.SECOND and F.Rows(fam.SECOND["m"])
    if two:
        gate[two.rows] = fam.SECOND["thr"]
    m2 = two.rows if two else 0
    res = {}
    for lik in (False, True):
        f, st0, aux = fam.handle(B, dtype, n, dialect)
        with f:
            inp = fam.mixed(st0, dtype, aux)
            f.set_gate(gate)
            if lik:
                f.loglik_enable()
                assert all((x == 0).all() for x in f.loglik())
            nis, dof = fam.call(f, inp, "nis")
            st1, app = f.get_state(), f.applied().astype(bool)
            if two:
                inp2 = two.readings(st1, dtype, seed=fam.SECOND["seed"])
                nis2, dof2 = two.call(f, inp2, "nis")
                assert f.applied().all()
                res[lik] = outs(f, np.stack([nis, nis2]), np.stack([dof, dof2]))
            else:
                res[lik] = outs(f, nis, dof)
            if lik:
                ll, rows, napp, nrej = f.loglik()
    assert same_rows(res[False], res[True])                          # the sums change no record, flag or output
    kinds = inp["kinds"]
    rej = (kinds == 0) & ~app
    assert app.sum() >= fam.MIN_APPLIED and rej.sum() >= 10
    assert np.array_equal(rows, fam.rows * app.astype(np.int64) + m2) and np.array_equal(napp, app.astype(np.int32) + bool(two))
    assert np.array_equal(nrej, rej.astype(np.int32))
    want = np.zeros(B)
    want[app] = -0.5 * (nis.astype(np.float64)[app] + fam.ref(st0, n, inp, fam.THR)[4][app] + fam.rows * math.log(2 * math.pi))
    summed = app
    if two:
        want += -0.5 * (nis2.astype(np.float64) + two.ref(st1, n, inp2)[4] + m2 * math.log(2 * math.pi))
        summed = np.ones(B, bool)
    err = np.abs(ll[summed] - want[summed]).max()
    print(f"{fam} f{dtype}: max |ll - sum (-1/2)(nis + ln det S + m ln 2 pi)| = {err:.3e}")
    assert err <= 1e-9 + NIS_TOL[dtype]
    assert (ll[~summed] == 0).all()                                   # (the untouched lanes among them)
    un = kinds != 0                                                    # untouched lanes: the first call moves no sum
    assert (rows[un] == m2).all() and (napp[un] == bool(two)).all() and (nrej[un] == 0).all()


# ---- independence ---------------------------------------------------------------------------------------------------------------------------------

def _job(fam, dtype=32, n=18, dialect=1):
    f, st0, aux = fam.handle(B, dtype, n, dialect)
    f.close()
    return st0, fam.cast(fam.mixed(st0, dtype, aux), dtype)


def _run(fam, st, inp, dtype=32, n=18, dialect=1, dev=False):
    """one gated update on a fresh handle holding exactly the state st; also returns the records as they were before it"""
    with BatchedFilter(len(st[0]), capi.default_params(dialect), device=0, dtype=dtype, nstate=n) as f:
        f.set_state(*st)
        before = dict(zip(NAMES, f.get_state()))
        fam.set_sensor(f)
        f.set_gate(fam.gate(fam.THR))
        nis, dof = fam.call(f, on_device(inp), "nis dev") if dev else fam.call(f, inp, "nis")
        f.sync()
        if dev:
            nis, dof = nis.cpu().numpy(), dof.cpu().numpy()
        return outs(f, nis, dof), before


@pytest.mark.parametrize("fam", FAMILIES)
def test_a_filter_is_itself_wherever_it_stands(fam):
    st0, inp = _job(fam)
    v0, _ = _run(fam, st0, inp)
    assert 0 < v0["applied"].sum() < B
    pi = permutation()
    assert same_rows(v0, _run(fam, [x[pi] for x in st0], {k: v[pi] for k, v in inp.items()})[0], rows=pi)
    # two handles cut inside a tile; the second reads SLICES of the whole job's device arrays, off the 16-byte boundary
    dev = on_device(inp)
    for part in ragged_cut():
        lo, hi = part[0], part[-1] + 1
        if lo:
            assert all(dev[k][lo:hi].data_ptr() % 16 != 0 for k in fam.keys)
        assert same_rows(v0, _run(fam, [x[part] for x in st0], {k: v[lo:hi] for k, v in dev.items()}, dev=True)[0], rows=part)


@pytest.mark.parametrize("fam", FAMILIES)
def test_a_clean_lane_among_broken_records_keeps_its_bits(fam):
    st0, inp = _job(fam)
    v0, _ = _run(fam, st0, inp)
    S, form = poison_set()
    nom, rot, P = poisoned_state(st0[0], st0[1], st0[2], S, form)
    bad = {k: v.copy() for k, v in inp.items()}
    bad[fam.keys[0]].reshape(B, -1)[S[form == 3], 0] = np.nan        # form (d): the input is broken, not the record
    if fam.NEG_COV_VAR is not None:
        # form (c): depth's variances (2.5e-5 .. 4e-4) straddle the prior's H P H' (0.85e-4 .. 1.4e-4), and a negated covariance under
        # var = 4e-4 leaves S > 0: a lane the rule applies.  Under the smallest of the three every negated covariance gives S < 0.
        bad["var"][S[form == 2]] = fam.NEG_COV_VAR
    out, before = _run(fam, [nom.astype(np.float32), rot.astype(np.float32), P.astype(np.float32), st0[3]], bad)
    clean = np.setdiff1d(np.arange(B), S)
    assert 100 in clean and len(np.intersect1d(clean, np.arange(64, 128))) == 1          # a whole wave but one lane
    assert same_rows(v0, out, clean, clean)
    # A record of NaN (a: nis is NaN), one with a negated covariance (c: no positive pivot) and a broken reading (d) are not applied.
    # An infinite position with variances of 1e30 (b) and a zero rotation (e) leave S finite with positive pivots: the header's rule
    # -- pivots > 0 and nis <= thr[rows] -- decides those, lane by lane.  Whatever is not applied keeps its bytes.
    usable = fam.usable(bad)
    for k in (0, 2, 3):
        assert (out["applied"][S[form == k]] == 0).all(), k
    ac = S[(form == 0) | (form == 2)]
    assert (out["dof"][ac] == fam.rows * usable[ac]).all() and np.isnan(out["nis"][S[form == 0]][usable[S[form == 0]]]).all()
    kept = S[out["applied"][S] == 0]
    assert len(kept) >= len(S) * 3 // 5
    assert same_rows(before, {k: out[k] for k in NAMES}, kept, kept)
