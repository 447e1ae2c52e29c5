"""GPU suite: per-filter process and measurement noise (fbus_ekf_set_noise*, fbus_ekf_get_noise).  A table of G = 5 distinct rows
(x0.1 .. x10 of the defaults in every column) given round-robin, so that every wave mixes rows: filter b must equal, bit for bit, a
handle whose fbus_params hold row b mod G, on every per-call route; a table equal to the handle's own parameters must change
nothing; the windows with a table must equal their frames run one by one; a sweep on the land recording must reproduce B = 1
replays of each row; the NIS must follow the filter's own R."""
import math
import os

import numpy as np
import pytest
import torch

from fbus_ekf import BatchedFilter, capi, gating, noise, replay, synth
from support import (B_ODD, G, J, SIZE, aa2q, assert_twin, imu, perturbed_setup, r32, rows_of, run_twins, same_state, state_of,
                     to_device, truth_scene, update_call, with_row)
from util import state_rel_err, state_rel_err_literal

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
def pose_inputs(B, M, nom, prm, dtype):
    ids, pos, quat = synth.marker_frame(0, B, 0, M, nom, prm)
    if dtype == 32:
        pos, quat = r32(pos), r32(quat)
    return ids, pos, quat


# ---- 1. twin bit-equality, every per-call route -------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [32, 64])
@pytest.mark.parametrize("dialect,nstate", [(0, 18), (1, 15)])
@pytest.mark.parametrize("K", [1, 7])
def test_predict_equals_its_twins(K, dialect, nstate, dtype):
    prm, state = state_of(B_ODD, dtype, nstate, dialect)
    a, w, dt = imu(B_ODD, K, state[0], dtype)
    step = (lambda f: f.predict(a[0], w[0], dt[:1])) if K == 1 else (lambda f: f.predict_n(a, w, dt))
    assert_twin(*run_twins(B_ODD, prm, dtype, nstate, state, step))


@pytest.mark.parametrize("dtype,nstate", [(32, 15), (64, 18), (64, 15)])
def test_parked_predict_n_equals_its_twins(dtype, nstate):
    """predict_n at a job of >= 2048 waves (the policy batch): the parked K-step loop on both sides.  (fp32 N = 18 runs the
    one-wave loop with a table: compared with its one-wave twin in test_predict_equals_its_twins)"""
    prm, state = state_of(B_ODD, dtype, nstate, 0)
    a, w, dt = imu(B_ODD, 7, state[0], dtype)
    assert_twin(*run_twins(B_ODD, prm, dtype, nstate, state, lambda f: f.predict_n(a, w, dt), policy_batch=200000))


POSE = [(0, 18, 0, 0), (0, 18, 1, 0), (1, 18, 0, 0), (1, 18, 1, 0), (0, 15, 1, 1), (1, 15, 0, 1), (1, 18, 1, 1)]


@pytest.mark.parametrize("nis", [False, True])
@pytest.mark.parametrize("dtype", [32, 64])
@pytest.mark.parametrize("dialect,nstate,mode,joseph", POSE)
def test_pose_correct_equals_its_twins(dialect, nstate, mode, joseph, dtype, nis):
    prm, state = state_of(B_ODD, dtype, nstate, dialect)
    prm.cov_form = capi.COV_JOSEPH if joseph else capi.COV_SIMPLE
    ids, pos, quat = pose_inputs(B_ODD, 4, state[0], prm, dtype)
    skip = (np.arange(B_ODD) % 11 == 4).astype(np.uint8)

    def step(f):
        if nis:
            return f.correct_nis(ids, pos, quat, mode, skip)
        f.correct(ids, pos, quat, mode, skip)
        return None
    # the plain update of a tabled handle runs the NIS kernel: bit-equal but for fp64 C++-dialect stacked (nominal within 2e-15)
    near = (not nis) and dtype == 64 and dialect == 1 and mode == capi.MODE_STACKED
    assert_twin(*run_twins(B_ODD, prm, dtype, nstate, state, step), near_nominal=near)


@pytest.mark.parametrize("nis", [False, True])
@pytest.mark.parametrize("dtype", [32, 64])
@pytest.mark.parametrize("kind,mode,dialect,nstate", [("left", 1, 0, 18), ("stereo", 1, 1, 15), ("corners", 1, 0, 15),
                                                      ("corners", 0, 1, 18)])
def test_meas_updates_equal_their_twins(kind, mode, dialect, nstate, dtype, nis):
    prm, nom, rot, P, prev, ids, left, right = perturbed_setup(B_ODD, dtype, nstate, dialect, kind)
    skip = (np.arange(B_ODD) % 7 == 3).astype(np.uint8)
    step = lambda f: update_call(f, kind, ids, left, right, nis=nis, mode=mode, skip=skip)
    assert_twin(*run_twins(B_ODD, prm, dtype, nstate, (nom, rot, P, prev), step))


# ---- 2. identity table, set_noise(None) -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [32, 64])
def test_identity_table_changes_nothing(dtype):
    """65 536 filters: the untabled handle's own routes are the one-wave forms"""
    B, nstate, dialect = 65536, 18, 0
    prm, state = state_of(B, dtype, nstate, dialect)
    a, w, dt = imu(B, 7, state[0], dtype)
    ids, pos, quat = pose_inputs(B, 4, state[0], prm, dtype)
    _, pnom, prot, pP, pprev, pids, pleft, pright = perturbed_setup(B, dtype, nstate, dialect, "stereo")
    _, cnom, crot, cP, cprev, cids, cleft, cright = perturbed_setup(B, dtype, nstate, dialect, "corners")

    def run(f):
        f.predict(a[0], w[0], dt[:1])
        f.predict_n(a, w, dt)
        f.correct(ids, pos, quat, capi.MODE_STACKED)
        f.correct(ids, pos, quat, capi.MODE_NEAREST)
        out = [f.get_state()]
        f.set_state(pnom, prot, pP, pprev)
        update_call(f, "left", pids, pleft, pright)
        update_call(f, "stereo", pids, pleft, pright)
        out.append(f.get_state())
        f.set_state(cnom, crot, cP, cprev)
        update_call(f, "corners", cids, cleft, cright, mode=capi.MODE_STACKED)
        update_call(f, "corners", cids, cleft, cright, mode=capi.MODE_NEAREST)
        out.append(f.get_state())
        return out

    with BatchedFilter(B, prm, dtype=dtype, nstate=nstate) as f0:
        f0.set_state(*state)
        ref = run(f0)
    with BatchedFilter(B, prm, dtype=dtype, nstate=nstate) as f1:
        f1.set_state(*state)
        f1.set_noise(noise.from_params(prm, B))
        np.testing.assert_array_equal(f1.get_noise(), noise.from_params(prm, B))
        got = run(f1)
    for x, y in zip(got, ref):
        assert same_state(x, y)
    # set_noise(None): back to the existing kernels (a handle never given a table)
    with BatchedFilter(B_ODD, prm, dtype=dtype, nstate=nstate) as f2, BatchedFilter(B_ODD, prm, dtype=dtype, nstate=nstate) as f3:
        _, st = state_of(B_ODD, dtype, nstate, dialect)
        a2, w2, dt2 = imu(B_ODD, 7, st[0], dtype)
        i2, p2, q2 = pose_inputs(B_ODD, 4, st[0], prm, dtype)
        for f in (f2, f3):
            f.set_state(*st)
        f2.set_noise(rows_of(prm)[np.arange(B_ODD) % G])
        f2.set_noise(None)
        with pytest.raises(capi.FbusError):
            f2.get_noise()
        for f in (f2, f3):
            f.predict_n(a2, w2, dt2)
            f.correct(i2, p2, q2, capi.MODE_STACKED)
        assert same_state(f2.get_state(), f3.get_state())


# ---- 3. oracle parity per row ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [32, 64])
def test_rows_match_the_oracle(dtype):
    from replay_ref import OracleEngine
    from util import PLAIN_TOL, assert_parity
    B, M = 320, 4
    for dialect in (0, 1):
        prm, state = state_of(B, dtype, 18, dialect)
        rows = rows_of(prm)
        g = np.arange(B) % G
        a, w, dt = imu(B, 1, state[0], dtype)
        ids, pos, quat = pose_inputs(B, M, state[0], prm, dtype)
        with BatchedFilter(B, prm, dtype=dtype, nstate=18) as f:
            f.set_state(*state)
            f.set_noise(rows[g])
            f.predict(a[0], w[0], dt)
            got_p = f.get_state()
            f.correct(ids, pos, quat, capi.MODE_STACKED)
            got_c = f.get_state()
        for k in range(G):
            sel = g == k
            n = int(sel.sum())
            eng = OracleEngine(n, dialect, 18)
            for i in range(4):
                eng.orc.prm.q_diag[i] = float(rows[k, i])
            eng.orc.prm.r_pos, eng.orc.prm.r_quat = float(rows[k, 4]), float(rows[k, 5])
            eng.set_state(*(np.asarray(x)[sel] for x in state))
            eng.predict(a[0][sel], w[0][sel], dt)
            assert_parity([np.asarray(x)[sel] for x in got_p], eng.get_state(), dtype, f"predict row {k} dialect {dialect}")
            eng.correct(ids[sel], pos[sel], quat[sel], capi.MODE_STACKED)
            # fp32: the rows with r_pos x 0.1 pull the state 10x harder than the defaults the gates were set for, and the tiny
            # bias block's per-block figure reaches 4e-4 (its twin with that r_pos in fbus_params is the same bit for bit, test 1)
            assert_parity([np.asarray(x)[sel] for x in got_c], eng.get_state(), dtype, f"correct row {k} dialect {dialect}",
                          plain_tol=1e-3 if dtype == 32 else PLAIN_TOL)


# ---- 4. windows and trajectories with a table -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [32, 64])
def test_windows_equal_their_frames(dtype):
    B, F, K, M, nstate = B_ODD, 4, 3, 4, 18
    prm, state = state_of(B, dtype, nstate, 0)
    rows = rows_of(prm)[np.arange(B) % G]
    a, w, dt = imu(B, F * K, state[0], dtype)
    kc = [K] * F
    ids = np.zeros((F, B, M), np.int32)
    pos = np.zeros((F, B, M, 3))
    quat = np.zeros((F, B, M, 4))
    for f in range(F):
        ids[f], pos[f], quat[f] = pose_inputs(B, M, state[0], prm, dtype)
    _, pnom, prot, pP, pprev, pids, pleft, pright = perturbed_setup(B, dtype, nstate, 0, "left")
    pix_ids = np.stack([pids] * F)
    pix_left = np.stack([pleft] * F)
    dtt = np.tile(dt[:K], F)
    with BatchedFilter(B, prm, dtype=dtype, nstate=nstate) as win, BatchedFilter(B, prm, dtype=dtype, nstate=nstate) as one:
        for h in (win, one):
            h.set_state(*state)
            h.set_noise(rows)
        npd = win.np_dtype
        traj = win.frames(kc, to_device(a, npd), to_device(w, npd), to_device(dtt, npd), to_device(ids, np.int32), to_device(pos, npd),
                          to_device(quat, npd), capi.MODE_STACKED, record=True)
        torch.cuda.synchronize()
        traj = [t.cpu().numpy() for t in traj]
        snaps = []
        for f in range(F):
            one.predict_n(a[f * K:(f + 1) * K], w[f * K:(f + 1) * K], dt[:K])
            one.correct(ids[f], pos[f], quat[f], capi.MODE_STACKED)
            one.sync()
            snaps.append([t.cpu().numpy() for t in one.snapshot()])
        assert same_state(win.get_state(), one.get_state())
        for f in range(F):
            for x, y in zip(traj, snaps[f]):
                assert np.array_equal(x[f], y)
        for h in (win, one):
            h.set_state(pnom, prot, pP, pprev)
        traj = win.frames_meas(kc, to_device(a, npd), to_device(w, npd), to_device(dtt, npd), to_device(pix_ids, np.int32),
                               to_device(pix_left, npd), record=True)
        torch.cuda.synchronize()
        traj = [t.cpu().numpy() for t in traj]
        snaps = []
        for f in range(F):
            one.predict_n(a[f * K:(f + 1) * K], w[f * K:(f + 1) * K], dt[:K])
            update_call(one, "left", pids, pleft, None)
            snaps.append([t.cpu().numpy() for t in one.snapshot()])
        assert same_state(win.get_state(), one.get_state())
        for f in range(F):
            for x, y in zip(traj, snaps[f]):
                assert np.array_equal(x[f], y)


# ---- 5. a noise sweep on the recording ------------------------------------------------------------------------------------------
def test_sweep_on_the_recording():
    d = np.load(os.path.join(GOLD, "recordings.npz"))
    imu_, image = d["land_imu"], d["land_image"]
    t = image[:, 0]
    keep = ~(((t > t[0] + 8.0) & (t < t[0] + 8.4)) | ((t > t[0] + 20.0) & (t < t[0] + 20.25)))
    image = image[keep]
    prm = capi.default_params(0)
    rows = rows_of(prm)
    B = 320
    for dtype, tol in ((64, 1e-9), (32, None)):
        ends = []
        for k in range(G):
            with BatchedFilter(1, with_row(prm, rows[k]), dtype=dtype) as f1:
                ref, _ = replay.replay(f1, imu_, image, with_row(prm, rows[k]))
            ends.append(ref[-1])
        with BatchedFilter(B, prm, dtype=dtype) as flt:
            flt.set_noise(rows[np.arange(B) % G])
            replay.replay_windowed(flt, imu_, image, prm)
            nom, rot, P, _ = flt.get_state()
        spread = min(state_rel_err_literal(ends[i][1:20][None], ends[j][1:20][None]) for i in range(G) for j in range(G) if i != j)
        for b in range(B):
            en, eP = ends[b % G][1:20], ends[b % G][29:].reshape(18, 18)
            lit = state_rel_err_literal(nom[b:b + 1].astype(np.float64), en[None])
            sig = state_rel_err(nom[b:b + 1].astype(np.float64), en[None], eP[None])
            if tol is not None:
                assert lit < tol and sig[0] < tol, (b, lit, sig)
            else:
                # test_recording_replay_through_frame_windows' fp32 band, the literal figure doubled: the row with r_pos x 0.1 and
                # q_theta x 10 pulls the state hardest and drifts 1.1e-4 (its sigma-aware figure 6e-4 is well inside)
                assert lit < 2e-4 and sig[0] < 3e-3, (b, lit, sig)
        print(f"sweep fp{dtype}: smallest row-to-row difference of the end states {spread:.2e}")
        assert spread > 1e-3                    # an ignored table would fail the bands above by far


# ---- 6. the NIS follows the filter's own R --------------------------------------------------------------------------------------
def test_nis_tracks_r():
    B, M, n = 3 * 8192, 4, 1024
    prm = capi.default_params(0)
    prm.marker_size = SIZE
    nom0, P0, prev, truth, _, ids, left, right = truth_scene(n, M, 11, 0.0)
    rep = B // n
    truth, ids, left, right, prev = (np.concatenate([a] * rep) for a in (truth, ids, left, right, prev))
    rng = np.random.default_rng(12)
    sig = math.sqrt(prm.r_pix)
    left = left + rng.normal(0, sig, left.shape)
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
    scale = np.array([0.25, 1.0, 4.0])
    g = np.arange(B) % 3
    table = noise.from_params(prm, B)
    table[:, 6] = prm.r_pix * scale[g]
    with BatchedFilter(B, prm, dtype=64, nstate=18) as f:
        f.set_state(nom, rot, np.broadcast_to(P, (B, 18, 18)).copy(), prev)
        f.set_noise(table)
        nis, dof = update_call(f, "left", ids, left, None, nis=True)
    means = []
    for k in range(3):
        ok = (dof > 0) & (g == k)
        means.append(float(np.mean(nis[ok] / dof[ok])))
        if k == 1:
            thr = gating.chi2_gate(0.99, int(dof.max()))
            above = float(np.mean(nis[ok] > thr[dof[ok]]))
            print(f"matched row: mean nis/dof {means[-1]:.4f}, above the 0.99 quantile {100 * above:.2f} % ({ok.sum()} filters)")
            assert 0.97 <= means[-1] <= 1.03
            assert 0.005 <= above <= 0.015
    print("mean nis/dof for r_pix x 0.25 / 1 / 4:", means)
    assert means[0] > means[1] > means[2]


# ---- 7. graph capture, validation, routes -------------------------------------------------------------------------------------
def test_graph_replay_sees_rewritten_values():
    B, dtype, nstate = B_ODD, 32, 18
    prm, state = state_of(B, dtype, nstate, 0)
    rows = rows_of(prm)
    a, w, dt = imu(B, 1, state[0], dtype)
    ids, pos, quat = pose_inputs(B, 4, state[0], prm, dtype)
    da, dw, ddt = to_device(a[0], np.float32), to_device(w[0], np.float32), to_device(dt[:1], np.float32)
    di, dp, dq = to_device(ids, np.int32), to_device(pos, np.float32), to_device(quat, np.float32)
    torch.cuda.synchronize()

    def step(f):
        f.predict(da, dw, ddt)
        f.correct(di, dp, dq, capi.MODE_STACKED)

    t1, t2 = rows[np.arange(B) % G], rows[(np.arange(B) + 2) % G]
    with BatchedFilter(B, prm, dtype=dtype, nstate=nstate) as gph, BatchedFilter(B, prm, dtype=dtype, nstate=nstate) as ref:
        for h in (gph, ref):
            h.set_state(*state)
        gph.set_noise(t1)
        gid = gph.graph_capture(lambda: step(gph))
        gph.set_state(*state)
        gph.graph_launch(gid)
        gph.sync()
        ref.set_noise(t1)
        step(ref)
        ref.sync()
        assert same_state(gph.get_state(), ref.get_state())
        gph.set_noise(t2)                      # rewritten in place: the graph reads the new values
        ref.set_noise(t2)
        gph.graph_launch(gid)
        gph.sync()
        step(ref)
        ref.sync()
        assert same_state(gph.get_state(), ref.get_state())


def test_validation_and_routes():
    B = B_ODD
    prm, state = state_of(B, 32, 18, 0)
    rows = rows_of(prm)[np.arange(B) % G]
    with BatchedFilter(B, prm, dtype=32, nstate=18) as f:
        f.set_team(4, 4)
        before = [f.launch_info(capi.INFO_ROLES_PREDICT, 1), f.launch_info(capi.INFO_ROLES_MEAS, 4)]
        assert max(before) > 1
        f.set_noise(rows)
        for c, v in ((0, -1e-3), (4, 0.0), (6, math.nan), (2, math.inf)):
            bad = rows.copy()
            bad[37, c] = v
            with pytest.raises(capi.FbusError) as e:
                f.set_noise(bad)
            assert "row 37" in str(e.value) and noise.COLUMNS[c] in str(e.value)
            np.testing.assert_array_equal(f.get_noise(), rows)          # the old table stays in force
        assert f.launch_info(capi.INFO_ROLES_PREDICT, 1) == 1 and f.launch_info(capi.INFO_ROLES_PREDICT, 7) == 1
        assert f.launch_info(capi.INFO_ROLES_MEAS, 4) == 1
        assert f.launch_info(capi.INFO_TEAM_FRAMES) == 0 and f.launch_info(capi.INFO_MEAS_SPLIT, 4) == 0
        f.set_noise(None)
        assert [f.launch_info(capi.INFO_ROLES_PREDICT, 1), f.launch_info(capi.INFO_ROLES_MEAS, 4)] == before
        # the device form, validated with torch
        f.set_noise(torch.from_numpy(rows).cuda())
        f.sync()
        np.testing.assert_array_equal(f.get_noise(), rows)
        bad = rows.copy()
        bad[5, 5] = -1.0
        with pytest.raises(ValueError):
            f.set_noise(torch.from_numpy(bad).cuda())
    with BatchedFilter(1, prm, dtype=32) as f1:
        with pytest.raises(capi.FbusError):
            f1.get_noise()
        with pytest.raises(capi.FbusError):
            f1.set_noise(np.array([[1e-3, 1e-3, 1e-3, 1e-3, 1e-2, 1e-2, 0.0]]))
        with pytest.raises(capi.FbusError):
            f1.get_noise()                     # a refused first table leaves none
