"""GPU suite: NIS output and chi-square gating of the pixel / corner updates (fbus_ekf_correct_pixels_nis*,
fbus_ekf_correct_corners_nis*, fbus_ekf_set_gate).  The NIS is held to r' (H P H' + R)^-1 r built in numpy from central differences
of the oracle's forward model (injection of MeasureUpdate.m:91-98: p += dp, q <- q (x) aa2q(dtheta)); the whole chain to its
chi-square statistics; the gate to its definition; and the entry points without a table to their twins, bit for bit."""
import math

import numpy as np
import pytest
import torch

import oracle_capi as oc
from fbus_ekf import capi, gating, synth
from support import (J, SIZE, aa2q, make_filter, measured_rows, perturbed_setup, pose_setup, predicted_rows, r32, same_state, to_device,
                     truth_scene, update_call, vp_tilted)
from util import assert_parity

pytestmark = pytest.mark.gpu
def nis_reference(nom, P, ids_b, left_b, right_b, prm, kind, eps=1e-6, vp=None, nearest=False):
    """(nis, dof) of one filter: r' (H P H' + R)^-1 r with H by central differences.  nearest (corner rows, Matlab dialect): the
    slot whose corner 0 is nearest (below 10 m) only"""
    vp = vp if vp is not None else oc.vision_params()
    if nearest:
        d = [np.linalg.norm(left_b[m, 0:3]) if ids_b[m] >= 0 else np.inf for m in range(len(ids_b))]
        m0 = int(np.argmin(d))
        keep = np.full(len(ids_b), -1, np.int32)
        if d[m0] < 10.0:
            keep[m0] = ids_b[m0]
        ids_b = keep
    h0, vis = predicted_rows(nom, ids_b, prm, vp, kind)
    y = measured_rows(ids_b, left_b, right_b, prm, kind)
    H = np.zeros((len(h0), 6))
    for j in range(6):
        col = []
        for s in (1.0, -1.0):
            d = np.zeros(6); d[j] = s * eps
            x = nom.copy()
            x[0:3] += d[0:3]
            x[6:10] = synth.qmul(nom[6:10][None], aa2q(d[3:6])[None])[0]
            col.append(predicted_rows(x, ids_b, prm, vp, kind)[0])
        H[:, j] = (col[0] - col[1]) / (2 * eps)
    H, r = H[vis], (y - h0)[vis]
    Rn = prm.r_pos if kind == "corners" else prm.r_pix
    S = H @ P[np.ix_(J, J)] @ H.T + Rn * np.eye(len(r))
    return float(r @ np.linalg.solve(S, r)), len(r)


KINDS = ["left", "stereo", "corners"]


@pytest.mark.parametrize("dtype", [32, 64])
@pytest.mark.parametrize("kind", KINDS)
def test_nis_matches_the_reference_algebra(kind, dtype):
    B, nstate = 4096, 18
    prm, nom, rot, P, prev, ids, left, right = perturbed_setup(B, dtype, nstate, 0, kind)
    with make_filter(B, prm, dtype, nstate, (nom, rot, P, prev)) as f:
        nom_p, _, P_p, _ = f.get_state()
        nis, dof = update_call(f, kind, ids, left, right, nis=True)
        applied = f.applied()
    worst = 0.0
    for b in range(256):
        ref, rdof = nis_reference(nom_p[b].astype(np.float64), P_p[b].astype(np.float64), ids[b], left[b], right[b], prm, kind)
        assert dof[b] == rdof, (b, dof[b], rdof)
        worst = max(worst, abs(nis[b] - ref) / max(ref, 1.0))
    print(f"{kind} fp{dtype}: worst |nis - ref| / max(ref, 1) = {worst:.2e}")
    assert applied[:256].all()
    assert worst < (1e-3 if dtype == 32 else 1e-6)


@pytest.mark.parametrize("roles", [0, 1])
@pytest.mark.parametrize("dtype", [32, 64])
@pytest.mark.parametrize("kind,mode,dialect,nstate", [("left", 1, 0, 18), ("stereo", 1, 1, 15), ("corners", 1, 0, 15),
                                                      ("corners", 0, 1, 18)])
def test_no_gate_is_the_twin_bit_for_bit(kind, mode, dialect, nstate, dtype, roles):
    """65 536 filters: the twin's own route is the one-wave kernel; 4096: the twin pinned to it (set_team(., 1))"""
    B = 65536 if roles == 0 else 4096
    prm, nom, rot, P, prev, ids, left, right = perturbed_setup(B, dtype, nstate, dialect, kind)
    skip = (np.arange(B) % 7 == 3).astype(np.uint8)
    with make_filter(B, prm, dtype, nstate, (nom, rot, P, prev), roles) as a, make_filter(B, prm, dtype, nstate, (nom, rot, P, prev), roles) as b, \
            make_filter(B, prm, dtype, nstate, (nom, rot, P, prev), roles) as c:
        update_call(a, kind, ids, left, right, mode=mode, skip=skip)
        nis, dof = update_call(b, kind, ids, left, right, nis=True, mode=mode, skip=skip)
        # NULL outputs
        di, dl, ds = to_device(ids, np.int32), to_device(left, c.np_dtype), to_device(skip, np.uint8)       # (alive until the sync)
        dr = to_device(right, c.np_dtype) if kind == "stereo" else None
        torch.cuda.synchronize()
        if kind == "corners":
            rc = c._lib.fbus_ekf_correct_corners_nis_dev(c._h, ids.shape[1], c._p(di), c._p(dl), None, capi.VIS_CORNERS3D, mode,
                                                         c._p(ds), None, None)
        else:
            rc = c._lib.fbus_ekf_correct_pixels_nis_dev(c._h, ids.shape[1], c._p(di), c._p(dl), c._p(dr), c._p(ds), None, None)
        c.sync()
        assert rc == 0
        sa, sb, sc = a.get_state(), b.get_state(), c.get_state()
        aa, ab, ac = a.applied(), b.applied(), c.applied()
    assert same_state(sa, sb) and same_state(sa, sc)
    assert np.array_equal(aa, ab) and np.array_equal(aa, ac)
    assert np.all(dof[skip == 1] == 0) and np.all(nis[skip == 1] == 0)
    assert np.all((dof > 0) == (ab == 1))


@pytest.mark.parametrize("kind", ["left", "stereo"])
def test_nis_is_chi_square_distributed(kind):
    """truth scenes with pixel noise sqrt(r_pix), the filter state truth (-) dx with dx ~ N(0, P): nis / dof has mean 1 and 1 % of
    the filters lie above the 0.99 quantile of their dof.  sigma_p = 5 mm, sigma_theta = 2.5 mrad: at 2 cm / 10 mrad the flat-port
    projection is no longer linear over dx, and the exact r' S^-1 r of the numpy reference itself averages 1.19 per row there"""
    B, M, n = 8192, 4, 1024
    prm = capi.default_params(0)
    prm.marker_size = SIZE
    nom0, P0, prev, truth, _, ids, left, right = truth_scene(n, M, 11, 0.0)
    rep = B // n
    truth, ids, left, right, prev = (np.concatenate([a] * rep) for a in (truth, ids, left, right, prev))
    rng = np.random.default_rng(12)
    sig = math.sqrt(prm.r_pix)
    left = left + rng.normal(0, sig, left.shape)
    right = right + rng.normal(0, sig, right.shape)
    P = np.array(np.diag(np.repeat(np.asarray(list(prm.p0_diag), float), 3)[:18]))
    sp, st = 0.005, 0.0025
    P[np.ix_(J[:3], J[:3])] = np.eye(3) * sp ** 2
    P[np.ix_(J[3:], J[3:])] = np.eye(3) * st ** 2
    dx = rng.normal(size=(B, 6)) * np.array([sp] * 3 + [st] * 3)
    nom = truth.copy()
    nom[:, 0:3] -= dx[:, 0:3]
    for b in range(B):
        nom[b, 6:10] = synth.qmul(truth[b, 6:10][None], aa2q(-dx[b, 3:6])[None])[0]
    rot = synth.q2R(nom[:, 6:10]).reshape(B, 9)
    for dtype in (32, 64):
        with make_filter(B, prm, dtype, 18, (nom, rot, np.broadcast_to(P, (B, 18, 18)).copy(), prev)) as f:
            nis, dof = update_call(f, kind, ids, r32(left) if dtype == 32 else left, r32(right) if dtype == 32 else right, nis=True)
        ok = dof > 0
        ratio = float(np.mean(nis[ok] / dof[ok]))
        thr = gating.chi2_gate(0.99, int(dof.max()))
        above = float(np.mean(nis[ok] > thr[dof[ok]]))
        print(f"{kind} fp{dtype}: mean nis/dof {ratio:.4f}, above the 0.99 quantile {100 * above:.2f} % ({ok.sum()} filters)")
        assert 0.97 <= ratio <= 1.03
        assert 0.005 <= above <= 0.015


@pytest.mark.parametrize("B", [4096, 65536])
@pytest.mark.parametrize("kind", ["left", "corners"])
def test_the_gate_rejects_exactly_nis_above_its_threshold(kind, B):
    dtype, nstate = 32, 18
    prm, nom, rot, P, prev, ids, left, right = perturbed_setup(B, dtype, nstate, 0, kind)
    bad = np.arange(B) % 8 == 5
    left = left.copy()
    # one corner of slot 0 30 sigma off in every coordinate (a corner on a reflection; a rigid shift of all four would be taken
    # up by the prior's pose uncertainty)
    if kind == "left":
        left[bad, 0, 0:2] += 30 * math.sqrt(prm.r_pix)
    else:
        left[bad, 0, 0:3] += 30 * math.sqrt(prm.r_pos)
    thr = gating.chi2_gate(0.999)
    with make_filter(B, prm, dtype, nstate, (nom, rot, P, prev)) as g, make_filter(B, prm, dtype, nstate, (nom, rot, P, prev)) as u:
        before = g.get_state()
        g.set_gate(thr)
        nis, dof = update_call(g, kind, ids, left, right, nis=True)
        after, ag = g.get_state(), g.applied()
        update_call(u, kind, ids, left, right, nis=True)
        ungated, au = u.get_state(), u.applied()
    rej = (ag == 0) & (dof > 0)
    assert np.array_equal(rej, (dof > 0) & (nis > thr[dof]))
    assert rej[bad & (dof > 0)].all()
    clean = ~bad & (dof > 0)
    assert rej[clean].mean() <= 0.01
    for x, y, z in zip(after, before, ungated):
        assert np.array_equal(x[rej], y[rej])          # rejected: the record as it was (prev id included)
        assert np.array_equal(x[~rej], z[~rej])        # accepted: the update without a table
    assert np.array_equal(ag[~rej], au[~rej])


def test_validation_and_graph_replay():
    B, dtype, nstate, kind = 4096, 32, 18, "left"
    prm, nom, rot, P, prev, ids, left, right = perturbed_setup(B, dtype, nstate, 0, kind)
    with make_filter(B, prm, dtype, nstate, (nom, rot, P, prev)) as f:
        before = f.get_state()
        with pytest.raises(capi.FbusError):
            f.set_gate([math.inf, 1.0, float("nan")])
        with pytest.raises(capi.FbusError):
            f.set_gate([math.inf, -1.0])
        with pytest.raises(capi.FbusError):
            f.set_gate(np.full(capi.GATE_MAX_DOF + 2, math.inf))
        f.set_gate(gating.chi2_gate(0.999, 31))         # M = 4, left camera: dof up to 32 -- one entry short
        with pytest.raises(capi.FbusError):
            update_call(f, kind, ids, left, right, nis=True)
        with pytest.raises(capi.FbusError):
            update_call(f, "corners", ids, np.zeros((B, 4, 12)), None, nis=True)     # corners stacked: up to 48
        assert same_state(f.get_state(), before)
        f.set_gate(gating.chi2_gate(0.999, 32))
        di, dl = to_device(ids, np.int32), to_device(left, np.float32)
        nis_d = torch.empty(B, dtype=torch.float32, device="cuda")
        dof_d = torch.empty(B, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()                        # (the raw calls below do not order against torch's stream)
        run = lambda: f._check(f._lib.fbus_ekf_correct_pixels_nis_dev(f._h, 4, f._p(di), f._p(dl), None, None, f._p(nis_d),
                                                                      f._p(dof_d)), "nis_dev")
        # set_gate inside a capture is refused
        def cap():
            run()
            assert f._lib.fbus_ekf_set_gate(f._h, 0, None) == 1
        gid = f.graph_capture(cap)
        f.set_state(*before)
        f.graph_launch(gid)
        f.sync()
        g_state, g_app, g_nis, g_dof = f.get_state(), f.applied(), nis_d.cpu().numpy(), dof_d.cpu().numpy()
        f.set_state(*before)
        run()
        f.sync()
        assert same_state(f.get_state(), g_state) and np.array_equal(f.applied(), g_app)
        assert np.array_equal(nis_d.cpu().numpy(), g_nis) and np.array_equal(dof_d.cpu().numpy(), g_dof)


# ---- tilted port, corner nearest mode, small launches, host-pointer forms -----------------------------------------------------------

@pytest.mark.parametrize("dtype", [32, 64])
@pytest.mark.parametrize("kind", ["left", "stereo"])
def test_tilted_port_nis_and_twin(kind, dtype):
    """the general-normal kernels (NZ = false; the left camera as CAM = 1 with the IMU-frame rows): NIS against the reference with
    the same normal, and no table == the twin's one-wave kernel bit for bit"""
    B, nstate = 4096, 18
    prm, nom, rot, P, prev, ids, left, right = perturbed_setup(B, dtype, nstate, 0, kind, tilted=True)
    with make_filter(B, prm, dtype, nstate, (nom, rot, P, prev), 1) as a, make_filter(B, prm, dtype, nstate, (nom, rot, P, prev), 1) as b:
        nom_p, _, P_p, _ = b.get_state()
        update_call(a, kind, ids, left, right)
        nis, dof = update_call(b, kind, ids, left, right, nis=True)
        assert same_state(a.get_state(), b.get_state()) and np.array_equal(a.applied(), b.applied())
    vp = vp_tilted()
    worst = 0.0
    for k in range(64):
        ref, rdof = nis_reference(nom_p[k].astype(np.float64), P_p[k].astype(np.float64), ids[k], left[k], right[k], prm, kind, vp=vp)
        assert dof[k] == rdof
        worst = max(worst, abs(nis[k] - ref) / max(ref, 1.0))
    print(f"tilted {kind} fp{dtype}: worst |nis - ref| / max(ref, 1) = {worst:.2e}")
    assert worst < (1e-3 if dtype == 32 else 1e-6)


@pytest.mark.parametrize("dtype", [32, 64])
def test_corner_nearest_nis_matches_the_reference(dtype):
    B, nstate = 4096, 18
    prm, nom, rot, P, prev, ids, left, right = perturbed_setup(B, dtype, nstate, 0, "corners")
    with make_filter(B, prm, dtype, nstate, (nom, rot, P, prev)) as f:
        nom_p, _, P_p, _ = f.get_state()
        nis, dof = update_call(f, "corners", ids, left, right, nis=True, mode=capi.MODE_NEAREST)
    worst = 0.0
    for k in range(128):
        ref, rdof = nis_reference(nom_p[k].astype(np.float64), P_p[k].astype(np.float64), ids[k], left[k], None, prm, "corners",
                                  nearest=True)
        assert dof[k] == rdof == 12
        worst = max(worst, abs(nis[k] - ref) / max(ref, 1.0))
    print(f"corners nearest fp{dtype}: worst |nis - ref| / max(ref, 1) = {worst:.2e}")
    assert worst < (1e-3 if dtype == 32 else 1e-6)


@pytest.mark.parametrize("kind", ["left", "stereo", "corners"])
def test_small_launch_twin_agrees_to_the_single_step_gate(kind):
    """4096 filters with the default team choice: the twin divides the markers among several waves per tile (fp32 left: the split
    update), the _nis form runs one wave per tile -- the same update to rounding"""
    B, dtype, nstate = 4096, 32, 18
    prm, nom, rot, P, prev, ids, left, right = perturbed_setup(B, dtype, nstate, 0, kind)
    with make_filter(B, prm, dtype, nstate, (nom, rot, P, prev)) as a, make_filter(B, prm, dtype, nstate, (nom, rot, P, prev)) as b:
        update_call(a, kind, ids, left, right)
        update_call(b, kind, ids, left, right, nis=True)
        sa, sb = a.get_state(), b.get_state()
        assert np.array_equal(a.applied(), b.applied())
    e = assert_parity(sb, sa, dtype, f"_nis vs team twin, {kind}")
    print(f"{kind}: team twin vs _nis literal {e['literal']:.2e}")


@pytest.mark.parametrize("kind", ["pose", "left", "corners"])
def test_host_pointer_forms_equal_the_device_forms(kind):
    B, dtype, nstate = 4096, 32, 18
    if kind == "pose":
        prm, nom, rot, P, prev, ids, left, right = pose_setup(B, dtype, nstate, 1, False)
    else:
        prm, nom, rot, P, prev, ids, left, right = perturbed_setup(B, dtype, nstate, 0, kind)
    mode = capi.MODE_STACKED
    skip = (np.arange(B) % 5 == 1).astype(np.uint8)
    with make_filter(B, prm, dtype, nstate, (nom, rot, P, prev)) as a, make_filter(B, prm, dtype, nstate, (nom, rot, P, prev)) as b:
        gate = gating.chi2_gate(0.999, 64)
        a.set_gate(gate); b.set_gate(gate)
        nd, dd = update_call(a, kind, ids, left, right, nis=True, mode=mode, skip=skip)
        nh, dh = update_call(b, kind, ids, left, right, nis=True, mode=mode, skip=skip, host=True)
        assert isinstance(nh, np.ndarray) and dh.dtype == np.int32
        assert np.array_equal(nd, nh) and np.array_equal(dd, dh)
        assert same_state(a.get_state(), b.get_state()) and np.array_equal(a.applied(), b.applied())


# ---- the pose rows ------------------------------------------------------------------------------------------------------------------

def pose_nis_reference(orc, nom, rot, P, ids_b, pos_b, quat_b, used_ids, prm):
    """r' (H P H' + R)^-1 r over the 7 rows of each used marker (the oracle's h, H, r: MeasureUpdate.m:67-88 / filter.cpp:684-721)"""
    Hs, rs = [], []
    for m, mid in enumerate(ids_b):
        if mid not in used_ids:
            continue
        _, H, r = orc.measurement(nom, rot, int(mid), pos_b[m], quat_b[m])
        Hs.append(H); rs.append(r)
    H, r = np.concatenate(Hs), np.concatenate(rs)
    Rd = np.tile(np.array([prm.r_pos] * 3 + [prm.r_quat] * 4), len(rs))
    S = H @ P @ H.T + np.diag(Rd)
    return float(r @ np.linalg.solve(S, r)), float(np.sum(r * r / Rd))


@pytest.mark.parametrize("B", [4096, 65536])
@pytest.mark.parametrize("joseph", [False, True])
@pytest.mark.parametrize("dtype", [32, 64])
@pytest.mark.parametrize("nstate", [18, 15])
@pytest.mark.parametrize("dialect", [0, 1])
@pytest.mark.parametrize("mode", [capi.MODE_NEAREST, capi.MODE_STACKED])
def test_pose_nis_matches_the_reference_and_the_twin(mode, dialect, nstate, dtype, joseph, B):
    if B == 65536 and (nstate != 18 or joseph):
        pytest.skip("the full-chip launch: N = 18, simple form")
    prm, nom, rot, P, prev, ids, pos, quat = pose_setup(B, dtype, nstate, dialect, joseph)
    skip = (np.arange(B) % 9 == 4).astype(np.uint8)
    with make_filter(B, prm, dtype, nstate, (nom, rot, P, prev)) as a, make_filter(B, prm, dtype, nstate, (nom, rot, P, prev)) as b:
        st0 = b.get_state()
        update_call(a, "pose", ids, pos, quat, mode=mode, skip=skip)
        nis, dof = update_call(b, "pose", ids, pos, quat, nis=True, mode=mode, skip=skip)
        if dtype == 64 and dialect == 1 and mode == capi.MODE_STACKED:
            # the one route that is not bit-identical (include/fbus_ekf.h): fp64 records, C++ dialect, stacked -- the covariance is,
            # the nominal state differs in the last bits (<= 2e-15); held to the single-step gate
            sa, sb = a.get_state(), b.get_state()
            assert np.array_equal(sa[2], sb[2]) and np.array_equal(sa[3], sb[3])
            assert_parity(sb, sa, 64, "pose _nis vs twin, fp64 C++ stacked")
        else:
            assert same_state(a.get_state(), b.get_state())
        assert np.array_equal(a.applied(), b.applied())
        app = b.applied()
    n = 256
    nom_p, rot_p, P_p, prev_p = (np.ascontiguousarray(x[:n], np.float64 if x.dtype != np.int32 else np.int32) for x in st0)
    orc = oc.Oracle(dialect, nstate)
    mids = set(int(x) for x in synth.marker_table(prm)[0])
    if mode == capi.MODE_NEAREST:                       # the marker the oracle's correct picks
        eng_nom, eng_rot, eng_P, eng_prev = nom_p.copy(), rot_p.copy(), P_p.copy(), prev_p.copy()
        orc.correct(eng_nom, eng_rot, eng_P, eng_prev, ids[:n], pos[:n], quat[:n], mode)
    rows = 7 if dialect == 1 else 3
    worst, worst_abs = 0.0, 0.0
    for k in range(n):
        if skip[k]:
            assert nis[k] == 0 and dof[k] == 0
            continue
        if mode == capi.MODE_STACKED:
            used = [int(m) for m in ids[k] if int(m) in mids]
        elif dialect == 1:
            used = [int(eng_prev[k])] if app[k] else []
        else:
            d = [np.linalg.norm(pos[k, m]) if ids[k, m] >= 0 else np.inf for m in range(ids.shape[1])]
            m0 = int(np.argmin(d))
            used = [int(ids[k, m0])] if d[m0] < 10 and int(ids[k, m0]) in mids else []
        assert dof[k] == rows * len(used), (k, dof[k], used)
        if not used:
            continue
        ref, rr = pose_nis_reference(orc, nom_p[k], rot_p[k], P_p[k], ids[k], pos[k].astype(np.float64),
                                     quat[k].astype(np.float64), used, prm)
        tol = (1e-3 * max(ref, 1.0) + 1e-6 * rr) if dtype == 32 else (1e-8 * max(ref, 1.0) + 1e-12 * rr)
        assert abs(nis[k] - ref) <= tol, (k, nis[k], ref, rr)
        worst = max(worst, abs(nis[k] - ref) / max(ref, 1.0))
    print(f"pose mode {mode} dialect {dialect} N {nstate} fp{dtype} joseph {joseph} B {B}: worst |nis - ref| / max(ref, 1) = {worst:.2e}")


@pytest.mark.parametrize("B", [4096, 65536])
def test_pose_gate_rejects_exactly_nis_above_its_threshold(B):
    dtype, nstate = 32, 18
    prm, nom, rot, P, prev, ids, pos, quat = pose_setup(B, dtype, nstate, 1, False)
    bad = np.arange(B) % 8 == 5
    pos = pos.copy()
    pos[bad, 0, :] += 30 * math.sqrt(prm.r_pos)          # one marker's position 30 sigma off
    thr = gating.chi2_gate(0.999)
    with make_filter(B, prm, dtype, nstate, (nom, rot, P, prev)) as g, make_filter(B, prm, dtype, nstate, (nom, rot, P, prev)) as u:
        before = g.get_state()
        g.set_gate(thr)
        nis, dof = update_call(g, "pose", ids, pos, quat, nis=True)
        after, ag = g.get_state(), g.applied()
        update_call(u, "pose", ids, pos, quat, nis=True)
        ungated, au = u.get_state(), u.applied()
    rej = (ag == 0) & (dof > 0)
    assert np.array_equal(rej, (dof > 0) & (nis > thr[dof]))
    assert rej[bad & (dof > 0)].all()
    assert rej[~bad & (dof > 0)].mean() <= 0.01
    for x, y, z in zip(after, before, ungated):
        assert np.array_equal(x[rej], y[rej])
        assert np.array_equal(x[~rej], z[~rej])
    assert np.array_equal(ag[~rej], au[~rej])
