"""GPU suite: the per-filter innovation log-likelihood sums (fbus_ekf_loglik_*).  Every applied measurement update adds
ll = -1/2 (nis + log det S + rows ln 2 pi), S = H P H' + R, to its filter's sum.  Held to the dense S of the numpy references of
tests/test_nis_gpu.py; the records, applied, nis and dof to the same call with accumulation off, bit for bit; the counters to their
definition; the sums of every entry point to the per-call sequence; and the point of it all: the sums rank noise hypotheses."""
import math
import os

import numpy as np
import pytest
import torch

import oracle_capi as oc
from fbus_ekf import BatchedFilter, capi, gating, noise, replay, synth
from loglik_ref import LN2PI, dense_pixels, dense_pose, tol_m2ll
from support import J, SIZE, aa2q, make_filter, perturbed_setup, pose_setup, r32, same_state, to_device, truth_scene, update_call
from util import assert_parity

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _sums(f):
    ll, rows, app, rej = f.loglik()
    assert ll.dtype == np.float64 and rows.dtype == np.int64 and app.dtype == np.int32 and rej.dtype == np.int32
    return ll, rows, app, rej


# ---- 1. against the dense reference -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [32, 64])
@pytest.mark.parametrize("kind", ["left", "stereo", "corners"])
def test_pixel_and_corner_loglik_matches_the_dense_reference(kind, dtype):
    B, nstate = 4096, 18
    prm, nom, rot, P, prev, ids, left, right = perturbed_setup(B, dtype, nstate, 0, kind)
    skip = (np.arange(B) % 9 == 4).astype(np.uint8)
    with make_filter(B, prm, dtype, nstate, (nom, rot, P, prev)) as f:
        with pytest.raises(capi.FbusError):
            f.loglik()                                  # before the first enable
        f.loglik_enable(True)
        f.loglik_reset()
        nom_p, _, P_p, _ = f.get_state()
        nis, dof = update_call(f, kind, ids, left, right, nis=True, skip=skip)
        applied = f.applied()
        ll, rows, app, rej = _sums(f)
        ll_d, rows_d, app_d, rej_d = f.loglik(device=True)
        f.sync()
        assert np.array_equal(ll_d.cpu().numpy(), ll) and np.array_equal(rows_d.cpu().numpy(), rows)
        assert np.array_equal(app_d.cpu().numpy(), app) and np.array_equal(rej_d.cpu().numpy(), rej)
    assert np.array_equal(app, applied.astype(np.int32)) and np.all(rej == 0)
    assert np.array_equal(rows, np.where(applied == 1, dof, 0).astype(np.int64))
    assert np.all(ll[skip == 1] == 0) and np.all(rows[skip == 1] == 0) and np.all(app[skip == 1] == 0)
    worst, worst_mut = 0.0, math.inf
    for b in range(256):
        if skip[b]:
            continue
        nr, ld, nrow, lnr = dense_pixels(nom_p[b].astype(np.float64), P_p[b].astype(np.float64), ids[b], left[b], right[b], prm, kind)
        assert rows[b] == nrow == dof[b], (b, rows[b], nrow)
        ref = nr + ld + nrow * LN2PI
        tol = tol_m2ll(dtype, False, nr, ld)
        err = abs(-2.0 * ll[b] - ref)
        worst = max(worst, err / tol)
        assert err <= tol, (b, -2.0 * ll[b], ref, tol)
        # the gate is sharp: a reference with half the Cholesky logarithms, or with one row's ln r left out, is refused
        for mut in (nr + (nrow * lnr + 0.5 * (ld - nrow * lnr)) + nrow * LN2PI, ref - lnr):
            worst_mut = min(worst_mut, abs(-2.0 * ll[b] - mut) / tol)
            assert abs(-2.0 * ll[b] - mut) > tol, (b, mut, ref)
    print(f"{kind} fp{dtype}: worst |-2 ll - ref| / tol = {worst:.3f}; nearest mutated reference at {worst_mut:.1f} tol")


@pytest.mark.parametrize("joseph", [False, True])
@pytest.mark.parametrize("dtype", [32, 64])
@pytest.mark.parametrize("nstate", [18, 15])
@pytest.mark.parametrize("dialect", [0, 1])
@pytest.mark.parametrize("mode", [capi.MODE_NEAREST, capi.MODE_STACKED])
def test_pose_loglik_matches_the_dense_reference(mode, dialect, nstate, dtype, joseph):
    B = 4096
    prm, nom, rot, P, prev, ids, pos, quat = pose_setup(B, dtype, nstate, dialect, joseph)
    skip = (np.arange(B) % 9 == 4).astype(np.uint8)
    with make_filter(B, prm, dtype, nstate, (nom, rot, P, prev)) as f:
        f.loglik_enable(True)
        f.loglik_reset()
        st0 = f.get_state()
        nis, dof = update_call(f, "pose", ids, pos, quat, nis=True, mode=mode, skip=skip)
        app_u8 = f.applied()
        ll, rows, app, rej = _sums(f)
    assert np.array_equal(app, app_u8.astype(np.int32)) and np.all(rej == 0)
    n = 256
    nom_p, rot_p, P_p, prev_p = (np.ascontiguousarray(x[:n], np.float64 if x.dtype != np.int32 else np.int32) for x in st0)
    orc = oc.Oracle(dialect, nstate)
    mids = set(int(x) for x in synth.marker_table(prm)[0])
    if mode == capi.MODE_NEAREST:
        eng = [nom_p.copy(), rot_p.copy(), P_p.copy(), prev_p.copy()]
        orc.correct(eng[0], eng[1], eng[2], eng[3], ids[:n], pos[:n], quat[:n], mode)
    per = 7 if dialect == 1 else 3
    worst, worst_mut = 0.0, math.inf
    for k in range(n):
        if skip[k]:
            assert ll[k] == 0 and rows[k] == 0 and app[k] == 0 and rej[k] == 0
            continue
        if mode == capi.MODE_STACKED:
            used = [int(m) for m in ids[k] if int(m) in mids]
        elif dialect == 1:
            used = [int(eng[3][k])] if app_u8[k] else []
        else:
            d = [np.linalg.norm(pos[k, m]) if ids[k, m] >= 0 else np.inf for m in range(ids.shape[1])]
            m0 = int(np.argmin(d))
            used = [int(ids[k, m0])] if d[m0] < 10 and int(ids[k, m0]) in mids else []
        # rows of S: all seven of each used marker in BOTH dialects; dof: the rows with a residual (Matlab: 3)
        assert dof[k] == per * len(used) and rows[k] == 7 * len(used), (k, dof[k], rows[k], used)
        if not used:
            assert ll[k] == 0 and app[k] == 0
            continue
        nr, ld, nrow, rr = dense_pose(orc, nom_p[k], rot_p[k], P_p[k], ids[k], pos[k].astype(np.float64), quat[k].astype(np.float64), used, prm)
        assert nrow == rows[k]
        ref = nr + ld + nrow * LN2PI
        tol = tol_m2ll(dtype, True, nr, ld, rr)
        err = abs(-2.0 * ll[k] - ref)
        worst = max(worst, err / tol)
        assert err <= tol, (k, -2.0 * ll[k], ref, tol)
        lnR = len(used) * (3 * math.log(prm.r_pos) + 4 * math.log(prm.r_quat))
        for mut in (nr + (lnR + 0.5 * (ld - lnR)) + nrow * LN2PI, ref - math.log(prm.r_quat)):
            worst_mut = min(worst_mut, abs(-2.0 * ll[k] - mut) / tol)
            assert abs(-2.0 * ll[k] - mut) > tol, (k, mut, ref)
    print(f"pose mode {mode} dialect {dialect} N {nstate} fp{dtype} joseph {joseph}: worst |-2 ll - ref| / tol = {worst:.3f}; "
          f"nearest mutated reference at {worst_mut:.1f} tol")


# ---- 2. the records do not change ---------------------------------------------------------------------------------------------------

def _table(prm, B, col):
    return noise.grid(prm, B, **{col: [0.25, 0.5, 1.0, 2.0, 4.0]})[0]


@pytest.mark.parametrize("tabled", [False, True])
@pytest.mark.parametrize("B", [4096, 65536])
@pytest.mark.parametrize("dtype", [32, 64])
@pytest.mark.parametrize("kind,mode,dialect,nstate", [("left", 1, 0, 18), ("stereo", 1, 1, 15), ("corners", 1, 0, 15),
                                                      ("corners", 0, 1, 18)])
def test_pixel_and_corner_records_are_untouched(kind, mode, dialect, nstate, dtype, B, tabled):
    prm, nom, rot, P, prev, ids, left, right = perturbed_setup(B, dtype, nstate, dialect, kind)
    skip = (np.arange(B) % 7 == 3).astype(np.uint8)
    with make_filter(B, prm, dtype, nstate, (nom, rot, P, prev)) as a, make_filter(B, prm, dtype, nstate, (nom, rot, P, prev)) as b:
        if tabled:
            t = _table(prm, B, "r_pos" if kind == "corners" else "r_pix")
            a.set_noise(t); b.set_noise(t)
        b.loglik_enable(True)
        na, da = update_call(a, kind, ids, left, right, nis=True, mode=mode, skip=skip)
        nb, db = update_call(b, kind, ids, left, right, nis=True, mode=mode, skip=skip)
        assert same_state(a.get_state(), b.get_state())
        assert np.array_equal(a.applied(), b.applied())
        assert np.array_equal(na, nb) and np.array_equal(da, db)
        ll, rows, app, rej = _sums(b)
        assert np.array_equal(app, b.applied().astype(np.int32)) and np.array_equal(rows, np.where(app == 1, db, 0))
        if not tabled:
            with pytest.raises(capi.FbusError):
                b.get_noise()                           # the handle's own row in the table buffer is not "a table"


# every route at 4096 filters; the full-chip launch for N = 18, simple form (the cases tests/test_nis_gpu.py runs there)
POSE_ROUTES = [(nstate, joseph, B) for nstate in (18, 15) for joseph in (False, True) for B in (4096, 65536)
               if B == 4096 or (nstate == 18 and not joseph)]


@pytest.mark.parametrize("tabled", [False, True])
@pytest.mark.parametrize("nstate,joseph,B", POSE_ROUTES)
@pytest.mark.parametrize("dtype", [32, 64])
@pytest.mark.parametrize("dialect", [0, 1])
@pytest.mark.parametrize("mode", [capi.MODE_NEAREST, capi.MODE_STACKED])
def test_pose_records_are_untouched(mode, dialect, dtype, nstate, joseph, B, tabled):
    prm, nom, rot, P, prev, ids, pos, quat = pose_setup(B, dtype, nstate, dialect, joseph)
    skip = (np.arange(B) % 9 == 4).astype(np.uint8)
    with make_filter(B, prm, dtype, nstate, (nom, rot, P, prev)) as a, make_filter(B, prm, dtype, nstate, (nom, rot, P, prev)) as b:
        if tabled:
            t = _table(prm, B, "r_pos")
            a.set_noise(t); b.set_noise(t)
        b.loglik_enable(True)
        na, da = update_call(a, "pose", ids, pos, quat, nis=True, mode=mode, skip=skip)
        nb, db = update_call(b, "pose", ids, pos, quat, nis=True, mode=mode, skip=skip)
        if dtype == 64 and dialect == 1 and mode == capi.MODE_STACKED and not tabled:
            # the stated exception (include/fbus_ekf.h): fp64 records, C++ dialect, stacked -- handle a runs the untabled kernel, b
            # the tabled one: covariance bit-equal, nominal state to the single-step gate
            sa, sb = a.get_state(), b.get_state()
            assert np.array_equal(sa[2], sb[2]) and np.array_equal(sa[3], sb[3])
            assert_parity(sb, sa, 64, "pose _nis, accumulation on vs off, fp64 C++ stacked")
        else:
            assert same_state(a.get_state(), b.get_state())
        assert np.array_equal(a.applied(), b.applied())
        assert np.array_equal(na, nb) and np.array_equal(da, db)


# ---- 3. the gate --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["left", "corners", "pose"])
def test_a_rejected_update_counts_as_rejected_and_nothing_else(kind):
    B, dtype, nstate = 4096, 32, 18
    bad = np.arange(B) % 8 == 5
    if kind == "pose":
        prm, nom, rot, P, prev, ids, left, right = pose_setup(B, dtype, nstate, 1, False)
        left = left.copy()
        left[bad, 0, :] += 30 * math.sqrt(prm.r_pos)
    else:
        prm, nom, rot, P, prev, ids, left, right = perturbed_setup(B, dtype, nstate, 0, kind)
        left = left.copy()
        if kind == "left":
            left[bad, 0, 0:2] += 30 * math.sqrt(prm.r_pix)
        else:
            left[bad, 0, 0:3] += 30 * math.sqrt(prm.r_pos)
    thr = gating.chi2_gate(0.999)
    with make_filter(B, prm, dtype, nstate, (nom, rot, P, prev)) as g:
        g.set_gate(thr)
        g.loglik_enable(True)
        nis, dof = update_call(g, kind, ids, left, right, nis=True)
        ag = g.applied()
        ll, rows, app, rej = _sums(g)
    rejected = (ag == 0) & (dof > 0)
    assert rejected[bad & (dof > 0)].all() and rejected.sum() >= bad.sum() * 0.9
    assert np.array_equal(rej, rejected.astype(np.int32))
    assert np.all(ll[rejected] == 0) and np.all(rows[rejected] == 0) and np.all(app[rejected] == 0)
    assert np.all(app[~rejected & (dof > 0)] == 1) and np.all(rej[~rejected] == 0)
    assert np.all(ll[app == 1] != 0)


# ---- 4. accumulation is a sum -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,dtype", [("left", 32), ("stereo", 64), ("pose", 32), ("pose", 64)])
def test_accumulation_is_a_sum_and_enable_zero_freezes_it(kind, dtype):
    B, nstate = 4096, 18
    if kind == "pose":
        prm, nom, rot, P, prev, ids, left, right = pose_setup(B, dtype, nstate, 0, False)
    else:
        prm, nom, rot, P, prev, ids, left, right = perturbed_setup(B, dtype, nstate, 0, kind)
    rng = np.random.default_rng(5)
    conv = r32 if dtype == 32 else (lambda a: a)
    sig = 1e-3 if kind == "pose" else 2e-4
    lefts = [left] + [conv(left + rng.normal(0, sig, left.shape)) for _ in range(2)]
    with make_filter(B, prm, dtype, nstate, (nom, rot, P, prev)) as a, make_filter(B, prm, dtype, nstate, (nom, rot, P, prev)) as b:
        a.loglik_enable(True); b.loglik_enable(True)
        single = []
        for l in lefts:
            update_call(a, kind, ids, l, right, nis=True)
            b.loglik_reset()
            update_call(b, kind, ids, l, right, nis=True)
            single.append(_sums(b))
            assert same_state(a.get_state(), b.get_state())      # the twin is fed the same states
        ll, rows, app, rej = _sums(a)
        assert np.array_equal(ll, (single[0][0] + single[1][0]) + single[2][0])
        assert np.array_equal(rows, single[0][1] + single[1][1] + single[2][1])
        assert np.array_equal(app, single[0][2] + single[1][2] + single[2][2]) and app.max() == 3
        # enable(0): the sums stay while the records go on changing
        a.loglik_enable(False)
        before = a.get_state()
        update_call(a, kind, ids, lefts[1], right, nis=True)
        assert not same_state(a.get_state(), before)
        assert all(np.array_equal(x, y) for x, y in zip(_sums(a), (ll, rows, app, rej)))
        a.loglik_reset()
        assert all(np.all(x == 0) for x in _sums(a))


# ---- 5. every door ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["left", "pose"])
def test_every_entry_point_feeds_the_same_sums(kind):
    """30 frames of K = 2 IMU samples and one update (the same inputs every frame; the state moves on): per-call _dev, host-pointer,
    the fused frame entry point, the 30-frame window (without and with trajectory rows) and a captured graph of 15 frames replayed
    twice.  With accumulation on all of them run predict_n + the per-call update: the sums are equal bit for bit."""
    B, dtype, nstate, F, K = 4096, 32, 18, 30, 2
    if kind == "pose":
        prm, nom, rot, P, prev, ids, left, right = pose_setup(B, dtype, nstate, 0, False)
    else:
        prm, nom, rot, P, prev, ids, left, right = perturbed_setup(B, dtype, nstate, 0, kind)
    acc, gyr = synth.imu_samples(0, B, 0, K, nom)
    acc, gyr = r32(acc).astype(np.float32), r32(gyr).astype(np.float32)
    dt = np.full(K, 0.005, np.float32)
    ids32, l32 = np.ascontiguousarray(ids, np.int32), np.ascontiguousarray(left, np.float32)
    q32 = np.ascontiguousarray(right, np.float32) if kind == "pose" else None
    d_acc, d_gyr, d_dt, d_ids, d_l = to_device(acc), to_device(gyr), to_device(dt), to_device(ids32), to_device(l32)
    d_q = to_device(q32) if kind == "pose" else None
    rep = lambda t: t[None].expand(F, *t.shape).contiguous()
    w_acc, w_gyr, w_dt = d_acc.repeat(F, 1, 1), d_gyr.repeat(F, 1, 1), d_dt.repeat(F)
    kc = np.full(F, K, np.int32)
    torch.cuda.synchronize()

    def update_dev(f):
        if kind == "pose":
            f.correct(d_ids, d_l, d_q, capi.MODE_STACKED)
        else:
            f.correct_pixels(d_ids, d_l, None)

    def per_call(f, n=F):
        for _ in range(n):
            f.predict_n(d_acc, d_gyr, d_dt, K=K)
            update_dev(f)

    def host(f):
        for _ in range(F):
            f.predict_n(acc, gyr, dt, K=K)
            if kind == "pose":
                f.correct(ids32, l32, q32, capi.MODE_STACKED)
            else:
                f.correct_pixels(ids32, l32, None)

    def fused(f):
        for _ in range(F):
            if kind == "pose":
                f.frame(d_acc, d_gyr, d_dt, d_ids, d_l, d_q, capi.MODE_STACKED, fused=True)
            else:
                f.frame_meas(d_acc, d_gyr, d_dt, d_ids, d_l, None)

    def window(f, record):
        if kind == "pose":
            f.frames(kc, w_acc, w_gyr, w_dt, rep(d_ids), rep(d_l), rep(d_q), capi.MODE_STACKED, record=record)
        else:
            f.frames_meas(kc, w_acc, w_gyr, w_dt, rep(d_ids), rep(d_l), None, record=record)

    def graph(f):
        gid = f.graph_capture(lambda: per_call(f, F // 2))
        f.graph_launch(gid)
        f.graph_launch(gid)

    results = {}
    for name, door in (("per_call", per_call), ("host", host), ("fused", fused), ("window", lambda f: window(f, False)),
                       ("window_traj", lambda f: window(f, True)), ("graph", graph)):
        with make_filter(B, prm, dtype, nstate, (nom, rot, P, prev)) as f:
            before = f.launch_policy(M=4, K=K)
            f.loglik_enable(True)
            on = f.launch_policy(M=4, K=K)
            assert on["roles_predict"] == 1 and on["roles_predict_n"] == 1 and on["roles_meas"] == 1
            assert on["team_frames"] is False and on["meas_split"] == 0
            door(f)
            f.sync()
            results[name] = (_sums(f), f.get_state())
            f.loglik_enable(False)
            assert f.launch_policy(M=4, K=K) == before
    ref_sums, ref_state = results["per_call"]
    assert np.all(ref_sums[2] == F) and np.all(ref_sums[3] == 0)
    for name, (sums, state) in results.items():
        assert same_state(state, ref_state), name
        for x, y in zip(sums, ref_sums):
            assert np.array_equal(x, y), name


# ---- 6. it ranks hypotheses ---------------------------------------------------------------------------------------------------------

def _chi_square_scene(G, n=1024, seed=11):
    """the scene of test_nis_is_chi_square_distributed (truth scenes, pixel noise sqrt(r_pix), state = truth - dx, dx ~ N(0, P),
    sigma_p 5 mm, sigma_theta 2.5 mrad), every scene repeated G times in a row: filter b runs hypothesis b % G on scene b // G"""
    prm = capi.default_params(0)
    prm.marker_size = SIZE
    _, _, prev, truth, _, ids, left, right = truth_scene(n, 4, seed, 0.0)
    rng = np.random.default_rng(seed + 1)
    sig = math.sqrt(prm.r_pix)
    left = left + rng.normal(0, sig, left.shape)
    right = right + rng.normal(0, sig, right.shape)
    P = np.array(np.diag(np.repeat(np.asarray(list(prm.p0_diag), float), 3)[:18]))
    sp, st = 0.005, 0.0025
    P[np.ix_(J[:3], J[:3])] = np.eye(3) * sp ** 2
    P[np.ix_(J[3:], J[3:])] = np.eye(3) * st ** 2
    dx = rng.normal(size=(n, 6)) * np.array([sp] * 3 + [st] * 3)
    nom = truth.copy()
    nom[:, 0:3] -= dx[:, 0:3]
    for b in range(n):
        nom[b, 6:10] = synth.qmul(truth[b, 6:10][None], aa2q(-dx[b, 3:6])[None])[0]
    rp = lambda a: np.repeat(a, G, axis=0)
    nom, ids, left, right, prev = rp(nom), rp(ids), rp(left), rp(right), rp(prev)
    rot = synth.q2R(nom[:, 6:10]).reshape(n * G, 9)
    return prm, nom, rot, np.broadcast_to(P, (n * G, 18, 18)).copy(), prev, ids, left, right


FACTORS = [2.0 ** e for e in range(-3, 4)]


def dense_hypothesis_totals(kind, nscenes=128, dtype=64):
    """the dense reference alone (no GPU): total ll of each of the 7 hypotheses r_pix * 2^(-3..3) over the first nscenes scenes"""
    G = len(FACTORS)
    prm, nom, rot, P, prev, ids, left, right = _chi_square_scene(G)
    if dtype == 32:
        nom, left, right = r32(nom), r32(left), r32(right)
    tot = np.zeros(G)
    for b in range(nscenes * G):
        nr, ld, nrow, _ = dense_pixels(nom[b], P[b], ids[b], left[b], right[b], prm, kind, r=prm.r_pix * FACTORS[b % G])
        tot[b % G] += -0.5 * (nr + ld + nrow * LN2PI)
    return tot


@pytest.mark.parametrize("dtype", [32, 64])
@pytest.mark.parametrize("kind", ["left", "stereo"])
def test_the_sums_rank_noise_hypotheses(kind, dtype):
    """G = 7 hypotheses r_pix * 2^(-3..3) through set_noise on the chi-square scene (1024 scenes x 7 filters): noise.best must return
    the factor-1 hypothesis, and the per-hypothesis totals over the first 128 scenes must agree with the dense numpy reference within
    the per-filter tolerance of the dense-reference test, summed.
    The dense reference alone, run on a CPU for this seed (dense_hypothesis_totals, fp64 inputs, first 128 scenes): the total at
    factor 1 exceeds its best neighbour (factor 2 in both) by 64.7 nats (left camera) and 191.3 nats (stereo)."""
    G = len(FACTORS)
    prm, nom, rot, P, prev, ids, left, right = _chi_square_scene(G)
    B = len(nom)
    table, hyp, hrows = noise.grid(prm, B, r_pix=FACTORS)
    assert np.array_equal(hyp, np.arange(B) % G) and hrows[3, 6] == prm.r_pix
    if dtype == 32:
        left, right = r32(left), r32(right)
    with make_filter(B, prm, dtype, 18, (nom, rot, P, prev)) as f:
        f.set_noise(table)
        f.loglik_enable(True)
        f.loglik_reset()
        st = f.get_state()
        update_call(f, kind, ids, left, right, nis=True)
        ll, rows, app, rej = _sums(f)
    assert np.all(app == 1)
    g_best, total = noise.best(ll, hyp, G)
    print(f"{kind} fp{dtype}: totals {np.array2string(total, precision=1)}; best factor {FACTORS[g_best]}, margin "
          f"{total[3] - max(total[2], total[4]):.1f} nats over {B // G} scenes")
    assert g_best == 3, (g_best, total)
    ns = 128
    ref, tol, got = np.zeros(G), np.zeros(G), np.zeros(G)
    for b in range(ns * G):
        nr, ld, nrow, _ = dense_pixels(st[0][b].astype(np.float64), st[2][b].astype(np.float64), ids[b], left[b], right[b], prm, kind,
                                       r=table[b, 6])
        assert rows[b] == nrow
        ref[b % G] += nr + ld + nrow * LN2PI
        tol[b % G] += tol_m2ll(dtype, False, nr, ld)
        got[b % G] += -2.0 * ll[b]
    print(f"{kind} fp{dtype}: worst |sum(-2 ll) - ref| / tol over the hypotheses = {np.max(np.abs(got - ref) / tol):.3f}")
    assert np.all(np.abs(got - ref) <= tol), (got, ref, tol)
    assert int(np.argmax(-0.5 * ref)) == 3


# ---- 7. replay ----------------------------------------------------------------------------------------------------------------------

WATER_MARKER_SIDE = 0.1142


@pytest.mark.parametrize("what", ["water_pixels", "land_pose"])
def test_replay_windowed_returns_the_sums_of_the_per_call_replay(what):
    """replay_windowed(loglik=True) on 256 filters against replay(loglik=True) stepping the same frames per call on one filter (fp64
    records).  The two runs agree to 1e-9 in the state at every frame (tests/test_trajectory_gpu.py: predict_n against per-sample
    predicts) where the posterior sigmas are 1e-4 and more, so every whitened residual agrees to 1e-5 relative and every log det S
    far better: the bound is 1e-4 (|ll| + rows) on the sums; rows, applied and rejected are exact, all 256 filters bit-equal."""
    d = np.load(os.path.join(GOLD, "recordings.npz"))
    prm = capi.default_params(0)
    if what == "water_pixels":
        imu, image, corners, nfr = d["water_imu"], d["water_image"], d["water_corners"], 100
        prm.marker_size = WATER_MARKER_SIDE
    else:
        imu, image, corners, nfr = d["land_imu"], d["land_image"], None, 100
    with BatchedFilter(1, prm, dtype=64) as f1:
        ref_states, _, ref = replay.replay(f1, imu, image, prm, max_frames=nfr, corners=corners, loglik=True)
    with BatchedFilter(256, prm, dtype=64) as flt:
        out = replay.replay_windowed(flt, imu, image, prm, max_frames=nfr, corners=corners, loglik=True)
        assert isinstance(out, tuple) and len(out) == 2
        sums = out[1]
        plain = replay.replay_windowed(flt, imu, image, prm, max_frames=10, corners=corners)
        assert isinstance(plain, int)
    ll, rows, app, rej = sums
    assert all(np.all(x == x[0]) for x in sums)
    assert rows[0] == ref[1][0] and app[0] == ref[2][0] and rej[0] == ref[3][0] == 0
    assert app[0] > 0.8 * len(ref_states)
    print(f"{what}: ll {ll[0]:.6f} (windowed) / {ref[0][0]:.6f} (per call), {app[0]} updates, {rows[0]} rows")
    assert abs(ll[0] - ref[0][0]) <= 1e-4 * (abs(ref[0][0]) + rows[0])
