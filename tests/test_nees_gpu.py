"""fbus_ekf_nees on the device against tests/nees_ref.py (the header restated in numpy): parity, calibration, independence of the filters
and the NaN / skip exits, placement in the batch, read-only, and the forms of the call.

Tolerance of the parity test: the kernel and the float64 path of the reference run the same formulas in the same precision but not in the
same order (elimination order p, theta, v, ...; FMA contraction; 1 / sqrt in place of the division), so they may differ by what either
differs from the exact value -- measured on the test's OWN inputs as the largest relative gap between the reference's float64 and longdouble
paths, per kind of output -- times 16 for the orders, and never below 1e-12.  The gaps are printed.  No bound here comes from the kernel.
The calibration bounds are those of tests/test_nees_cpu.py: derived from the chi-square law, 5 sigma."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import nees_ref
from fbus_ekf import capi, consistency, gating
from support import B_IND, imu, make_filter, permutation, pose_setup, same_rows, to_device

pytestmark = pytest.mark.gpu

B = 200                                     # three full 64-filter tiles and 8 lanes
_PREPARED = {}


def prepared(dtype, nstate):
    """(prm, state, truth) of B filters that went through two predicts and one stacked pose update -- a dense, correlated covariance --
    read back with get_state(); truth = estimate (+) dx, dx_i = sqrt(P_ii) z_i.  Computed once per (dtype, nstate) and never written."""
    key = (dtype, nstate)
    if key not in _PREPARED:
        prm, nom, rot, P, prev, ids, pos, quat = pose_setup(B, dtype, nstate, 0, False, 4)
        a, w, dt = imu(B, 2, nom, dtype)
        with make_filter(B, prm, dtype, nstate, (nom, rot, P, prev)) as f:
            f.predict_n(a, w, dt, K=2)
            f.correct(ids, pos, quat, capi.MODE_STACKED)
            st = f.get_state()
            assert f.applied().all()
        z = np.random.default_rng(100 + dtype + nstate).normal(size=(B, nstate))
        sd = np.sqrt(np.einsum("bii->bi", st[2].astype(np.float64)))
        truth = nees_ref.boxplus(st[0], sd * z)
        for x in st + (truth,):
            x.setflags(write=False)
        _PREPARED[key] = (prm, st, truth)
    return _PREPARED[key]


def run(f, truth, skip=None, host=False):
    """nees, err and lnp of one call as numpy arrays; the device form unless host"""
    if host:
        out = f.nees(np.ascontiguousarray(truth), None if skip is None else np.ascontiguousarray(skip, np.uint8), err=True, lnp=True)
    else:
        out = f.nees(to_device(truth, np.float64), to_device(skip, np.uint8), err=True, lnp=True)
        f.sync()
        out = tuple(o.cpu().numpy() for o in out)
    assert out[0].shape == (f.B, 8) and out[1].shape == (f.B, f.N) and out[2].shape == (f.B,)
    assert all(o.dtype == np.float64 for o in out)
    return dict(zip(("nees", "err", "lnp"), out))


def within(got, ref, tol):
    return bool((np.abs(got - ref) <= tol * np.abs(ref)).all())


# ---- 1. parity --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,nstate", [(32, 18), (32, 15), (64, 18), (64, 15)])
def test_parity_with_the_reference(dtype, nstate):
    prm, st, truth = prepared(dtype, nstate)
    r_nees, r_err, r_lnp = nees_ref.nees(st[0], st[2], truth)
    l_nees, l_err, l_lnp = nees_ref.nees(st[0], st[2], truth, dtype=np.longdouble)
    assert np.isfinite(r_nees).all() and np.isfinite(r_lnp).all()
    gaps = {"nees": nees_ref.rel_gap(r_nees, l_nees), "theta": nees_ref.rel_gap(r_err[:, 6:9], l_err[:, 6:9]), "lnp": nees_ref.rel_gap(r_lnp, l_lnp)}
    tol = {k: max(1e-12, 16 * g) for k, g in gaps.items()}
    with make_filter(B, prm, dtype, nstate, st) as f:
        got = run(f, truth)
    plain = [i for i in range(nstate) if not 6 <= i < 9]
    dev = {"nees": nees_ref.rel_gap(got["nees"], r_nees), "theta": nees_ref.rel_gap(got["err"][:, 6:9], r_err[:, 6:9]),
           "lnp": nees_ref.rel_gap(got["lnp"], r_lnp)}
    print(f"fp{dtype} N={nstate}: gap float64 / longdouble {gaps}, device against float64 {dev}, "
          f"cond(P) <= {np.linalg.cond(st[2].astype(np.float64)).max():.2e}")
    assert same_rows({"err": got["err"][:, plain]}, {"err": r_err[:, plain]})          # one exact subtraction: bit for bit
    assert within(got["err"][:, 6:9], r_err[:, 6:9], tol["theta"])
    assert within(got["nees"], r_nees, tol["nees"])
    assert within(got["lnp"], r_lnp, tol["lnp"])
    if nstate == 15:
        assert not got["nees"][:, capi.NEES_G].any()


# ---- 2. calibration on the device --------------------------------------------------------------------------------------------------------
def calibrated(col, dof, n):
    mean, share = float(col.mean()), float((col > gating.chi2_ppf(0.95, dof)).mean())
    bm, bs = 5 * math.sqrt(2 * dof / n), 5 * math.sqrt(0.05 * 0.95 / n)
    print(f"dof {dof}: mean {mean:.3f} against {dof} +- {bm:.3f}, share {share:.4f} against 0.05 +- {bs:.4f}")
    return abs(mean - dof) <= bm and abs(share - 0.05) <= bs


def test_calibration_before_and_after_a_depth_update():
    n, var = 8192, 1e-2
    nom, rot, P, prev, truth = nees_ref.calibration_inputs(n, 18, 1)
    prm = capi.default_params(0)
    d_truth = to_device(truth, np.float64)
    with make_filter(n, prm, 32, 18, (nom, rot, P, prev)) as f:
        prior = f.nees(d_truth)
        f.sync()
        prior = prior.cpu().numpy()
        assert np.isfinite(prior).all()
        assert all([calibrated(prior[:, c], dof, n) for c, dof in enumerate(consistency.nees_dof(18))])
        assert all(v["inside"] is not None for v in consistency.summary(prior, 18, 0.95).values())
        # one exactly linear row: the depth along z with zero lever, z = h(truth) + N(0, var)
        f.set_depth_sensor([0.0, 0.0, 1.0], 0.0, None)
        z = truth[:, 2] + math.sqrt(var) * np.random.default_rng(2).normal(size=n)
        f.correct_depth(to_device(z, np.float32), np.array([var]))
        f.sync()
        assert f.applied().all()
        post = f.nees(d_truth)
        f.sync()
        post = post.cpu().numpy()
    assert np.isfinite(post).all()
    assert (post[:, capi.NEES_P] != prior[:, capi.NEES_P]).mean() > 0.99           # the update moved the filters
    assert calibrated(post[:, capi.NEES_FULL], 18, n) and calibrated(post[:, capi.NEES_P], 3, n)


# ---- 3. independence and exits -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [32, 64])
def test_a_bad_filter_reports_its_own_nan_columns_and_reaches_no_other(dtype):
    nstate = 18
    prm, st, truth = prepared(dtype, nstate)
    F, POSE, P_, V, TH, BA, BG, G = range(8)
    nom, rot, P = (np.array(x) for x in st[:3])
    tr = np.array(truth)
    nom[3, 0] = np.nan                      # the record's p
    nom[70, 14] = np.nan                    # the record's bg alone
    P[130, 4, 4] = -P[130, 4, 4]            # one negated diagonal element (v)
    tr[64] = np.nan                         # a NaN truth row
    tr[199, 6:10] = 0.0                     # a zero truth quaternion
    want = {3: {F, POSE, P_}, 70: {F, BG}, 130: {F, V}, 64: set(range(8)), 199: {F, POSE, TH}}
    skip = np.zeros(B, np.uint8)
    skip[[5, 127, 198]] = 1
    with make_filter(B, prm, dtype, nstate, st) as f:
        clean = run(f, truth)
        f.set_state(nom, rot, P, st[3])
        got = run(f, tr, skip)
    assert np.isfinite(clean["nees"]).all() and np.isfinite(clean["lnp"]).all()
    for b, cols in want.items():
        assert set(np.nonzero(np.isnan(got["nees"][b]))[0]) == cols, b
        assert np.isnan(got["lnp"][b])
        fin = [c for c in range(8) if c not in cols]
        assert same_rows({"nees": got["nees"][[b]][:, fin]}, {"nees": clean["nees"][[b]][:, fin]}), b      # the clean columns: as they were
    assert np.isnan(got["err"][3, 0]) and np.isfinite(got["err"][3, 1:]).all()
    assert np.isnan(got["err"][70, 13]) and np.isfinite(np.delete(got["err"][70], 13)).all()
    assert same_rows({"err": got["err"][[130]]}, {"err": clean["err"][[130]]})
    assert np.isnan(got["err"][64]).all()
    assert np.isnan(got["err"][199, 6:9]).all() and np.isfinite(np.delete(got["err"][199], [6, 7, 8])).all()
    sk = np.nonzero(skip)[0]
    assert not got["nees"][sk].any() and not got["err"][sk].any() and not got["lnp"][sk].any()
    rest = np.setdiff1d(np.arange(B), list(want) + list(sk))
    assert same_rows(got, clean, rest, rest)


# ---- 4. placement --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,nstate", [(32, 18), (64, 15)])
def test_a_filter_is_judged_the_same_whatever_its_place_or_batch(dtype, nstate):
    prm, st, truth = prepared(dtype, nstate)
    n = B_IND
    sub = lambda rows: tuple(np.ascontiguousarray(x[rows]) for x in st)
    with make_filter(n, prm, dtype, nstate, sub(np.arange(n))) as f:
        base = run(f, truth[:n])
        again = run(f, truth[:n])
    assert same_rows(base, again)
    assert same_rows(base, {k: v[:n] for k, v in _full(prm, st, truth, dtype, nstate).items()})
    pi = permutation(n)
    with make_filter(n, prm, dtype, nstate, sub(pi)) as f:
        assert same_rows(run(f, truth[pi]), base, None, pi)
    for m in (1, 63, 64, 65):
        with make_filter(m, prm, dtype, nstate, sub(np.arange(m))) as f:
            assert same_rows(run(f, truth[:m]), base, None, np.arange(m)), m
    with make_filter(1, prm, dtype, nstate, sub(np.array([100]))) as f:
        assert same_rows(run(f, truth[[100]]), base, None, np.array([100]))


def _full(prm, st, truth, dtype, nstate):
    with make_filter(B, prm, dtype, nstate, st) as f:
        return run(f, truth)


# ---- 5. read-only --------------------------------------------------------------------------------------------------------------------------
def test_the_call_writes_nothing_but_its_outputs():
    dtype, nstate = 32, 18
    prm, nom, rot, P, prev, ids, pos, quat = pose_setup(B, dtype, nstate, 0, False, 4)
    _, st, truth = prepared(dtype, nstate)
    with make_filter(B, prm, dtype, nstate, (nom, rot, P, prev)) as f:
        f.loglik_enable(True)
        f.correct_nis(ids, pos, quat, capi.MODE_STACKED)        # applied flags and likelihood sums that are not all zero
        _, _, total = f.records()

        def snap():
            buf = torch.empty(total, dtype=torch.uint8, device="cuda")
            f.copy_records(buf)
            f.sync()
            return buf.cpu().numpy()
        rec0, app0, lik0 = snap(), f.applied(), f.loglik()
        d = run(f, truth)
        h = run(f, truth, host=True)
        rec1, app1, lik1 = snap(), f.applied(), f.loglik()
    assert same_rows(d, h)
    assert np.array_equal(rec0, rec1) and np.array_equal(app0, app1) and app0.any()
    assert all(np.array_equal(x, y) for x, y in zip(lik0, lik1)) and lik0[1].any()


# ---- 6. forms ------------------------------------------------------------------------------------------------------------------------------
def test_forms_null_outputs_graph_replay_and_refusals():
    dtype, nstate = 32, 18
    prm, st, truth = prepared(dtype, nstate)
    skip = (np.arange(B) % 5 == 2).astype(np.uint8)
    with make_filter(B, prm, dtype, nstate, st) as f:
        lib, h, p = f._lib, f._h, f._p
        full = run(f, truth, skip)
        assert same_rows(full, run(f, truth, skip, host=True))         # the host form equals _dev bit for bit
        only = f.nees(np.array(truth))
        assert isinstance(only, np.ndarray) and same_rows({"nees": only}, {"nees": run(f, truth)["nees"]})
        d_truth, d_skip = to_device(np.array(truth), np.float64), to_device(skip, np.uint8)
        names, widths = ("nees", "err", "lnp"), (8, nstate, 1)
        torch.cuda.synchronize()                            # (the raw calls below do not order against torch's stream)
        for mask in range(8):                               # every subset of the outputs, the empty one included
            bufs = [torch.full((B, w), 77.0, dtype=torch.float64, device="cuda") for w in widths]
            torch.cuda.synchronize()
            args = [p(b) if mask >> i & 1 else None for i, b in enumerate(bufs)]
            assert lib.fbus_ekf_nees_dev(h, p(d_truth), p(d_skip), *args) == 0, mask
            f.sync()
            for i, (name, b) in enumerate(zip(names, bufs)):
                got = b.cpu().numpy().reshape(full[name].shape)
                assert same_rows({name: got}, {name: full[name]}) if mask >> i & 1 else (got == 77.0).all(), (mask, name)
            hb = [np.full((B, w), 77.0) for w in widths]
            assert lib.fbus_ekf_nees(h, p(np.array(truth)), p(skip), *[p(b) if mask >> i & 1 else None for i, b in enumerate(hb)]) == 0
            for i, (name, b) in enumerate(zip(names, hb)):
                got = b.reshape(full[name].shape)
                assert same_rows({name: got}, {name: full[name]}) if mask >> i & 1 else (got == 77.0).all(), (mask, name)
        # refusals, each FBUS_ERR_INVALID with the entry point's name
        o = torch.full((B, 8), 77.0, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        recs, _, total = f.records()
        for fn, name in ((lib.fbus_ekf_nees_dev, b"fbus_ekf_nees_dev"), (lib.fbus_ekf_nees, b"fbus_ekf_nees")):
            assert fn(h, None, None, p(o), None, None) == 1 and name in lib.fbus_ekf_last_error(h)
            assert fn(None, p(d_truth), None, p(o), None, None) == 1
        for args in ((C.c_void_p(recs), None, None), (None, C.c_void_p(recs + total - 8), None), (None, None, C.c_void_p(recs + 1024))):
            assert lib.fbus_ekf_nees_dev(h, p(d_truth), None, *args) == 1
            assert b"fbus_ekf_nees_dev" in lib.fbus_ekf_last_error(h) and b"overlaps the records" in lib.fbus_ekf_last_error(h)
        f.sync()
        assert (o.cpu().numpy() == 77.0).all()              # nothing was launched
        # a captured _dev call reads the truth current at its replay
        o_err = torch.full((B, nstate), 77.0, dtype=torch.float64, device="cuda")
        o_lnp = torch.full((B,), 77.0, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        h_out = np.full((B, 8), 77.0)

        def cap():
            f._check(lib.fbus_ekf_nees_dev(h, p(d_truth), p(d_skip), p(o), p(o_err), p(o_lnp)), "nees_dev")
            assert lib.fbus_ekf_nees(h, p(np.array(truth)), None, p(h_out), None, None) == 1       # the host form cannot be captured
            assert b"fbus_ekf_nees" in lib.fbus_ekf_last_error(h)
        gid = f.graph_capture(cap)
        f.graph_launch(gid)
        f.sync()
        assert (h_out == 77.0).all()
        assert same_rows({"nees": o.cpu().numpy(), "err": o_err.cpu().numpy(), "lnp": o_lnp.cpu().numpy()}, full)
        other = nees_ref.boxplus(st[0], 0.5 * nees_ref.delta(st[0], truth, nstate))           # another truth, refilled in place
        d_truth.copy_(torch.from_numpy(other))
        torch.cuda.synchronize()
        f.graph_launch(gid)
        f.sync()
        replay = {"nees": o.cpu().numpy(), "err": o_err.cpu().numpy(), "lnp": o_lnp.cpu().numpy()}
        assert same_rows(replay, run(f, other, skip))
        assert not np.array_equal(replay["nees"], full["nees"])
