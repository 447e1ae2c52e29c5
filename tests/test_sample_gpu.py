"""fbus_ekf_sample on the device against tests/sample_ref.py (the header restated in numpy) and against fbus_ekf_nees itself: parity, the
closed loop sample -> nees, sigma points, calibration, the exits, read-only, placement in the batch, the forms of the call, and perturb().

Tolerances: the kernel and the float64 path of the reference run the same formulas in the same precision but not in the same order, so
they may differ by what either differs from the exact value.  That is measured on the test's OWN inputs -- parity: the largest relative
gap between the reference's float64 and longdouble paths, per kind of output; the loop and the moments: the gap of the reference's own
float64 loop against the exact identity (|xi|^2, Pi' L xi, P) -- times 16 for the orders, and never below 1e-12.  The gaps are printed.  No
bound here comes from the kernel.  The calibration bounds are those of tests/test_nees_cpu.py: derived from the chi-square law, 5 sigma."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import nees_ref
import sample_ref
from fbus_ekf import capi, consistency, gating, synth
from support import B_IND, imu, make_filter, permutation, pose_setup, same_rows, to_device

pytestmark = pytest.mark.gpu

B = 200                                     # three full 64-filter tiles and 8 lanes
S3 = 3
CASES = [(32, 18), (32, 15), (64, 18), (64, 15)]
_PREPARED = {}


def prepared(dtype, nstate):
    """(prm, state, xi) of B filters that went through two predicts and one stacked pose update -- a dense, correlated covariance -- read
    back with get_state(); xi (S3, B, N) standard normal.  Computed once per (dtype, nstate) and never written."""
    key = (dtype, nstate)
    if key not in _PREPARED:
        prm, nom, rot, P, prev, ids, pos, quat = pose_setup(B, dtype, nstate, 0, False, 4)
        a, w, dt = imu(B, 2, nom, dtype)
        with make_filter(B, prm, dtype, nstate, (nom, rot, P, prev)) as f:
            f.predict_n(a, w, dt, K=2)
            f.correct(ids, pos, quat, capi.MODE_STACKED)
            st = f.get_state()
            assert f.applied().all()
        xi = np.random.default_rng(300 + dtype + nstate).normal(size=(S3, B, nstate))
        for x in st + (xi,):
            x.setflags(write=False)
        _PREPARED[key] = (prm, st, xi)
    return _PREPARED[key]


def run(f, xi, skip=None, host=False):
    """state and drawn of one call as numpy arrays; the device form unless host"""
    if host:
        out = f.sample(np.ascontiguousarray(xi), None if skip is None else np.ascontiguousarray(skip, np.uint8), drawn=True)
    else:
        out = f.sample(to_device(np.ascontiguousarray(xi), np.float64), to_device(skip, np.uint8), drawn=True)
        f.sync()
        out = tuple(o.cpu().numpy() for o in out)
    assert out[0].shape == (len(xi), f.B, 19) and out[1].shape == (f.B,)
    assert out[0].dtype == np.float64 and out[1].dtype == np.uint8
    return {"state": np.ascontiguousarray(out[0].transpose(1, 0, 2)), "drawn": out[1]}         # the filters along axis 0


def nees_of(f, rows):
    """(cols (S, B, 3) = FULL, POSE, P, err (S, B, N)) of nees_dev with every row as truth"""
    cols, errs = [], []
    for s in range(len(rows)):
        n, e = f.nees(to_device(np.ascontiguousarray(rows[s]), np.float64), err=True)
        f.sync()
        cols.append(n.cpu().numpy()[:, [capi.NEES_FULL, capi.NEES_POSE, capi.NEES_P]])
        errs.append(e.cpu().numpy())
    return np.stack(cols), np.stack(errs)


def deltas(est, rows, N):
    return np.stack([nees_ref.delta(est, rows[s], N, np.longdouble) for s in range(len(rows))])


def within(got, ref, tol):
    return bool((np.abs(got - ref) <= tol * np.abs(ref)).all())


def tol_of(gap):
    return max(1e-12, 16 * gap)


def bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


# ---- 1. parity ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,nstate", CASES)
def test_parity_with_the_reference(dtype, nstate):
    prm, st, xi = prepared(dtype, nstate)
    r_rows, r_drawn, _ = sample_ref.sample(st[0], st[2], xi)
    l_rows, _, _ = sample_ref.sample(st[0], st[2], xi, dtype=np.longdouble)
    assert r_drawn.all() and np.isfinite(r_rows).all()
    with make_filter(B, prm, dtype, nstate, st) as f:
        got = run(f, xi)
    assert got["drawn"].all()
    g_rows = got["state"].transpose(1, 0, 2)
    dr, dl, dg = deltas(st[0], r_rows, nstate), deltas(st[0], l_rows, nstate), deltas(st[0], g_rows, nstate)
    plain = [i for i in range(nstate) if not 6 <= i < 9]
    th = [6, 7, 8]
    gaps = {"plain": nees_ref.rel_gap(dr[..., plain], dl[..., plain]), "theta": nees_ref.rel_gap(dr[..., th], dl[..., th])}
    dev = {"plain": nees_ref.rel_gap(dg[..., plain], dr[..., plain]), "theta": nees_ref.rel_gap(dg[..., th], dr[..., th])}
    print(f"fp{dtype} N={nstate}: gap float64 / longdouble {gaps}, device against float64 {dev}, "
          f"cond(P) <= {np.linalg.cond(st[2].astype(np.float64)).max():.2e}")
    assert within(dg[..., plain], dr[..., plain], tol_of(gaps["plain"]))
    assert within(dg[..., th], dr[..., th], tol_of(gaps["theta"]))
    assert np.abs(np.linalg.norm(g_rows[:, :, 6:10], axis=2) - 1).max() < 1e-15        # normalised in double
    if nstate == 15:                        # g of an N = 15 filter: the record's, bit for bit
        assert np.array_equal(bits(g_rows[:, :, 16:19]), bits(np.broadcast_to(st[0][:, 16:19].astype(np.float64), (S3, B, 3))))


# ---- 2. the closed loop: a drawn row as truth -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,nstate", CASES)
def test_nees_of_a_drawn_row_is_the_prefix_sums_of_xi_squared(dtype, nstate):
    prm, st, xi = prepared(dtype, nstate)
    want = sample_ref.prefix_sums(xi)
    want_err = sample_ref.delta(st[2], xi, np.longdouble)[0]
    r_cols, r_err = sample_ref.loop(st[0], st[2], xi)
    gaps = {"nees": max(nees_ref.rel_gap(r_cols[:, :, c], want[c]) for c in range(3)), "err": nees_ref.rel_gap(r_err, want_err)}
    with make_filter(B, prm, dtype, nstate, st) as f:
        got = run(f, xi)
        cols, err = nees_of(f, got["state"].transpose(1, 0, 2))
    dev = {"nees": max(nees_ref.rel_gap(cols[:, :, c], want[c]) for c in range(3)), "err": nees_ref.rel_gap(err, want_err)}
    print(f"fp{dtype} N={nstate}: the reference's loop against the identity {gaps}, the device's {dev}")
    for c in range(3):
        assert within(cols[:, :, c], want[c].astype(np.float64), tol_of(gaps["nees"])), c
    assert within(err, want_err.astype(np.float64), tol_of(gaps["err"]))


# ---- 3. sigma points ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,nstate", CASES)
def test_sigma_points_reproduce_the_mean_and_the_covariance(dtype, nstate):
    prm, st, _ = prepared(dtype, nstate)
    pts, w = consistency.sigma_points(nstate)
    xi = np.ascontiguousarray(np.broadcast_to(pts[:, None, :], (len(pts), B, nstate)))
    r_rows = sample_ref.sample(st[0], st[2], xi)[0]
    gm, gc = sample_ref.moment_gaps(st[0], st[2], r_rows, w)
    with make_filter(B, prm, dtype, nstate, st) as f:
        got = run(f, xi)
    assert got["drawn"].all()
    dm, dc = sample_ref.moment_gaps(st[0], st[2], got["state"].transpose(1, 0, 2), w)
    print(f"fp{dtype} N={nstate}: |sum w delta| / sigma: reference {gm:.2e}, device {dm:.2e}; "
          f"|sum w delta delta' - P| / sqrt(P_ii P_jj): reference {gc:.2e}, device {dc:.2e}")
    assert dm <= tol_of(gm) and dc <= tol_of(gc)


# ---- 4. calibration on the device ------------------------------------------------------------------------------------------------------------
def calibrated(col, dof, n):
    mean, share = float(col.mean()), float((col > gating.chi2_ppf(0.95, dof)).mean())
    bm, bs = 5 * math.sqrt(2 * dof / n), 5 * math.sqrt(0.05 * 0.95 / n)
    print(f"dof {dof}: mean {mean:.3f} against {dof} +- {bm:.3f}, share {share:.4f} against 0.05 +- {bs:.4f}")
    return abs(mean - dof) <= bm and abs(share - 0.05) <= bs


def test_states_drawn_on_the_device_are_calibrated_in_every_column():
    n = 8192
    nom, rot, P, prev, _ = nees_ref.calibration_inputs(n, 18, 1)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(5)
    with make_filter(n, capi.default_params(0), 32, 18, (nom, rot, P, prev)) as f:
        state, xi = consistency.draw(f, 2, gen)
        assert tuple(state.shape) == (2, n, 19) and tuple(xi.shape) == (2, n, 18)
        for s in range(2):
            nees = f.nees(state[s])
            f.sync()
            nees = nees.cpu().numpy()
            assert np.isfinite(nees).all()
            assert all([calibrated(nees[:, c], dof, n) for c, dof in enumerate(consistency.nees_dof(18))])


# ---- 5. exits ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,nstate", [(32, 18), (64, 15)])
def test_a_bad_filter_is_its_nominal_and_reaches_no_other(dtype, nstate):
    prm, st, xi = prepared(dtype, nstate)
    nom, rot, P = (np.array(x) for x in st[:3])
    P[130, 2, 11] = P[130, 11, 2] = np.nan          # a NaN in P
    nom[130, 4] = -0.0                              # (a nominal row is copied, not recomputed: the sign of a zero stays)
    P[70, 1, 1] = -P[70, 1, 1]                      # a negative diagonal element of the p block
    P[199] = 0.0                                    # nothing to factorise in the last filter of the tail tile
    skip = np.zeros(B, np.uint8)
    skip[[5, 127]] = 1
    bad = [5, 127, 130, 70, 199]
    x2 = np.array(xi)
    x2[1, 64] = np.nan                              # a NaN row of xi: that row of that filter and nothing else
    with make_filter(B, prm, dtype, nstate, st) as f:
        clean = run(f, xi)
        f.set_state(nom, rot, P, st[3])
        got = run(f, x2, skip)
        nominal = f.get_state()[0].astype(np.float64)
    assert clean["drawn"].all() and np.isfinite(clean["state"]).all()
    assert not got["drawn"][bad].any() and got["drawn"][np.setdiff1d(np.arange(B), bad)].all()
    for b in bad:
        for s in range(S3):
            assert np.array_equal(bits(got["state"][b, s]), bits(nominal[b])), (b, s)
    assert not np.isfinite(got["state"][64, 1, :16]).any()
    if nstate == 18:
        assert not np.isfinite(got["state"][64, 1]).any()
    assert np.array_equal(bits(got["state"][64, [0, 2]]), bits(clean["state"][64, [0, 2]]))
    rest = np.setdiff1d(np.arange(B), bad + [64])
    assert same_rows(got, clean, rest, rest)


# ---- 6. read-only -----------------------------------------------------------------------------------------------------------------------------
def test_the_call_writes_nothing_but_its_outputs():
    dtype, nstate = 32, 18
    prm, nom, rot, P, prev, ids, pos, quat = pose_setup(B, dtype, nstate, 0, False, 4)
    xi = prepared(dtype, nstate)[2]
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
        d = run(f, xi)
        h = run(f, xi, host=True)
        rec1, app1, lik1 = snap(), f.applied(), f.loglik()
    assert d["drawn"].all() and same_rows(d, h)
    assert np.array_equal(rec0, rec1) and np.array_equal(app0, app1) and app0.any()
    assert all(np.array_equal(x, y) for x, y in zip(lik0, lik1)) and lik0[1].any()


# ---- 7. placement -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,nstate", [(32, 18), (64, 15)])
def test_a_filter_draws_the_same_whatever_its_place_or_batch(dtype, nstate):
    prm, st, xi = prepared(dtype, nstate)
    n = B_IND
    sub = lambda rows: tuple(np.ascontiguousarray(x[rows]) for x in st)
    with make_filter(B, prm, dtype, nstate, st) as f:
        full = run(f, xi)
    with make_filter(n, prm, dtype, nstate, sub(np.arange(n))) as f:
        base = run(f, xi[:, :n])
        assert same_rows(base, run(f, xi[:, :n]))
    assert same_rows(base, {k: v[:n] for k, v in full.items()})
    pi = permutation(n)
    with make_filter(n, prm, dtype, nstate, sub(pi)) as f:
        assert same_rows(run(f, xi[:, pi]), base, None, pi)
    for m in (1, 63, 64, 65):
        with make_filter(m, prm, dtype, nstate, sub(np.arange(m))) as f:
            assert same_rows(run(f, xi[:, :m]), base, None, np.arange(m)), m
    with make_filter(1, prm, dtype, nstate, sub(np.array([100]))) as f:
        assert same_rows(run(f, xi[:, [100]]), base, None, np.array([100]))
    # and a row does not depend on how many rows the call draws
    with make_filter(n, prm, dtype, nstate, sub(np.arange(n))) as f:
        one = run(f, xi[1:2, :n])
    assert np.array_equal(bits(one["state"][:, 0]), bits(base["state"][:, 1]))


# ---- 8. forms ---------------------------------------------------------------------------------------------------------------------------------
def test_forms_null_outputs_graph_replay_and_refusals():
    dtype, nstate = 32, 18
    prm, st, xi = prepared(dtype, nstate)
    xi = np.array(xi)
    skip = (np.arange(B) % 5 == 2).astype(np.uint8)
    with make_filter(B, prm, dtype, nstate, st) as f:
        lib, h, p = f._lib, f._h, f._p
        full = run(f, xi, skip)
        assert same_rows(full, run(f, xi, skip, host=True))            # the host form equals _dev bit for bit
        assert np.array_equal(full["drawn"], 1 - skip)
        only = f.sample(xi)
        assert isinstance(only, np.ndarray) and np.array_equal(bits(only), bits(run(f, xi)["state"].transpose(1, 0, 2)))
        d_xi, d_skip = to_device(xi, np.float64), to_device(skip, np.uint8)
        want = {"state": full["state"].transpose(1, 0, 2), "drawn": full["drawn"]}
        torch.cuda.synchronize()                            # (the raw calls below do not order against torch's stream)
        for mask in range(4):                               # every subset of the outputs, the empty one included
            bufs = [torch.full((S3, B, 19), 77.0, dtype=torch.float64, device="cuda"), torch.full((B,), 77, dtype=torch.uint8, device="cuda")]
            torch.cuda.synchronize()
            assert lib.fbus_ekf_sample_dev(h, S3, p(d_xi), p(d_skip), *[p(b) if mask >> i & 1 else None for i, b in enumerate(bufs)]) == 0, mask
            f.sync()
            hb = [np.full((S3, B, 19), 77.0), np.full(B, 77, np.uint8)]
            assert lib.fbus_ekf_sample(h, S3, p(xi), p(skip), *[p(b) if mask >> i & 1 else None for i, b in enumerate(hb)]) == 0, mask
            for i, name in enumerate(("state", "drawn")):
                for got in (bufs[i].cpu().numpy(), hb[i]):
                    assert same_rows({name: got}, {name: want[name]}) if mask >> i & 1 else (got == 77).all(), (mask, name)
        # refusals, each FBUS_ERR_INVALID with the entry point's name; the order of the tests: handle, S, xi, overlap
        o = torch.full((S3, B, 19), 77.0, dtype=torch.float64, device="cuda")
        o_dr = torch.full((B,), 77, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        recs, _, total = f.records()
        err = lambda: lib.fbus_ekf_last_error(h)
        for fn, name in ((lib.fbus_ekf_sample_dev, b"fbus_ekf_sample_dev"), (lib.fbus_ekf_sample, b"fbus_ekf_sample")):
            assert fn(None, S3, p(d_xi), None, p(o), None) == 1
            for S in (0, -1, capi.SAMPLE_MAX + 1):
                assert fn(h, S, None, None, p(o), None) == 1 and name in err() and b"S must be" in err(), S
            assert fn(h, S3, None, None, p(o), None) == 1 and name in err() and b"xi is NULL" in err()
        for args in ((C.c_void_p(recs), None), (C.c_void_p(recs + total - 8), None), (None, C.c_void_p(recs + 1024))):
            assert lib.fbus_ekf_sample_dev(h, S3, p(d_xi), None, *args) == 1
            assert b"fbus_ekf_sample_dev" in err() and b"overlaps the records" in err()
        assert lib.fbus_ekf_sample_dev(h, 0, None, None, C.c_void_p(recs), None) == 1 and b"S must be" in err()
        assert lib.fbus_ekf_sample_dev(h, S3, None, None, C.c_void_p(recs), None) == 1 and b"xi is NULL" in err()
        with pytest.raises(ValueError):
            f.sample(xi[:, :B - 1])
        with pytest.raises(ValueError):
            f.sample(xi.astype(np.float32))
        f.sync()
        assert (o.cpu().numpy() == 77.0).all()              # nothing was launched
        # a captured _dev call reads the xi current at its replay
        h_out = np.full((S3, B, 19), 77.0)

        def cap():
            f._check(lib.fbus_ekf_sample_dev(h, S3, p(d_xi), p(d_skip), p(o), p(o_dr)), "sample_dev")
            assert lib.fbus_ekf_sample(h, S3, p(xi), None, p(h_out), None) == 1        # the host form cannot be captured
            assert b"fbus_ekf_sample" in err() and b"graph_begin" in err()
        gid = f.graph_capture(cap)
        f.graph_launch(gid)
        f.sync()
        assert (h_out == 77.0).all()
        assert same_rows({"state": o.cpu().numpy(), "drawn": o_dr.cpu().numpy()}, want)
        other = np.ascontiguousarray(-0.5 * xi[::-1])       # other coordinates, refilled in place
        d_xi.copy_(torch.from_numpy(other))
        torch.cuda.synchronize()
        f.graph_launch(gid)
        f.sync()
        replay = {"state": np.ascontiguousarray(o.cpu().numpy().transpose(1, 0, 2)), "drawn": o_dr.cpu().numpy()}
        assert same_rows(replay, run(f, other, skip))
        assert not np.array_equal(replay["state"], full["state"])


# ---- 9. perturb ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [32, 64])
def test_perturb_moves_the_filters_to_one_draw_and_nees_against_the_old_state_is_xi_squared(dtype):
    n, nstate = 8192, 18
    nom, rot, P, prev, _ = nees_ref.calibration_inputs(n, nstate, 1)
    nom = np.ascontiguousarray(np.broadcast_to(nom[7], (n, 19)))       # one shared truth: every filter starts on it
    rot = np.ascontiguousarray(np.broadcast_to(rot[7], (n, 9)))
    xi = np.random.default_rng(21).normal(size=(1, n, nstate))
    npd = np.float32 if dtype == 32 else np.float64
    cast = lambda rows: np.asarray(rows).astype(npd).astype(np.float64)
    skip = np.zeros(n, np.uint8)
    skip[[3, 4000]] = 1
    P = np.array(P)
    P[9] = -P[9]                                                # one filter that cannot be drawn
    stay = [3, 9, 4000]
    moved = np.setdiff1d(np.arange(n), stay)
    with make_filter(n, capi.default_params(0), dtype, nstate, (nom, rot, P, prev)) as f:
        before = f.get_state()
        d_xi = to_device(xi, np.float64)
        rows = f.sample(d_xi, to_device(skip, np.uint8))
        f.sync()
        rows = rows.cpu().numpy()[0]
        drawn = f.perturb(d_xi[0], to_device(skip, np.uint8))
        f.sync()
        drawn = drawn.cpu().numpy()
        after = f.get_state()
        nees = f.nees(to_device(nom, np.float64))
        f.sync()
        nees = nees.cpu().numpy()
    assert not drawn[stay].any() and drawn[moved].all()
    assert np.array_equal(bits(after[0].astype(np.float64)), bits(cast(rows)))                 # the nominal: the cast sample
    assert np.array_equal(after[2], before[2]) and np.array_equal(after[3], before[3])          # P and prev_id: bit-equal
    assert np.array_equal(after[1][stay], before[1][stay])                                      # a filter that stays keeps its rotation
    # rot: the rotation matrix of the record's quaternion, formed in double and rounded once.  Entries of size <= 1: half a spacing of
    # the record type at 1 for the one rounding, and 2e-15 for two float64 evaluations that differ in form (each under ten operations on
    # values <= 1 behind a normalisation: 16 x 2^-53 apiece at the most)
    q = after[0][moved, 6:10].astype(np.float64)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    assert np.abs(after[1][moved].astype(np.float64) - synth.q2R(q).reshape(-1, 9)).max() <= 0.5 * np.finfo(npd).eps + 2e-15
    # NEES of the old state against the perturbed filters: conj(q (x) Exp delta) (x) q = Exp(-delta) exactly, so FULL = |xi|^2
    want = sample_ref.prefix_sums(xi)[0][0]
    r_full = sample_ref.loop(nom[moved], P[moved], xi[:, moved], cast=cast)[0][0, :, 0]
    gap = nees_ref.rel_gap(r_full, want[moved])
    got = nees_ref.rel_gap(nees[moved, capi.NEES_FULL], want[moved])
    print(f"fp{dtype}: the reference's loop with the cast against |xi|^2 {gap:.2e}, the device's {got:.2e}")
    assert within(nees[moved, capi.NEES_FULL], want[moved].astype(np.float64), tol_of(gap))
    assert all([calibrated(nees[moved, c], dof, len(moved)) for c, dof in enumerate(consistency.nees_dof(nstate))])
