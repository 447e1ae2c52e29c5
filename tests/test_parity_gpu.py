"""GPU suite: the HIP path, called through the C ABI (ctypes), against the fp64 oracle.

Tolerances (BASELINE.json north_star): fp32 GPU vs fp64 oracle, state rel-err <= 1e-5,
covariance rel-err <= 1e-4 (max-norm relative), asserted per step (re-seeded from the
oracle) and over free-running windows of <= 100 frames; fp64 GPU vs oracle <= 1e-9.
Nothing here reads /root/reference.
"""
import os

import numpy as np
import pytest

import oracle_capi as oc
from fbus_ekf import BatchedFilter, capi, replay, synth
from replay_ref import OracleEngine
from support import DT, imu_of, markers_of, params_of, r32, state_batch
from util import (COV_BLOCK_TOL, COV_TOL, PLAIN_TOL, PLAIN_WINDOW_TOL, STATE_TOL, WINDOW_TOL, assert_parity, assert_window_parity, cov_rel_err,
                  cov_rel_err_blockwise, parity_errors, rot_rel_err, state_rel_err, state_rel_err_literal,
                  state_rel_err_plain)

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
def _check(flt, eng, dtype, what, state_tol=STATE_TOL, cov_tol=COV_TOL, plain_tol=PLAIN_TOL, cov_block_tol=COV_BLOCK_TOL):
    """the parity gate of tests/util.py (literal, sigma-aware and plain per-block state error, rotation, max-norm and
    block-wise covariance error, symmetry, marker id) between the device state and the oracle's"""
    e = assert_parity(flt.get_state(), eng.get_state(), dtype, what, state_tol, cov_tol, plain_tol, cov_block_tol)
    return e["sigma"], e["cov"]


# ------------------------------------------------------------------ single steps
@pytest.mark.parametrize("dtype", [32, 64])
@pytest.mark.parametrize("n", [18, 15])
@pytest.mark.parametrize("dialect", [0, 1])
def test_predict_single_step(dialect, n, dtype):
    B = 320                                   # five waves, last tile partial on purpose below
    B -= 7
    prm, nom, rot, P, prev = state_batch(B, dialect, n)
    acc, gyr = imu_of(0, B, 0, 1, nom)
    dt = r32(np.random.default_rng(3).uniform(0.001, 0.01, B))
    with BatchedFilter(B, prm, dtype=dtype, nstate=n) as flt:
        eng = OracleEngine(B, dialect, n)
        flt.set_state(nom, rot, P, prev)
        eng.set_state(nom, rot, P, prev)
        flt.predict(acc[0], gyr[0], dt)
        eng.predict(acc[0], gyr[0], dt)
        _check(flt, eng, dtype, "predict")
        # scalar dt form
        flt.predict(acc[0], gyr[0], DT)
        eng.predict(acc[0], gyr[0], DT)
        _check(flt, eng, dtype, "predict scalar dt")


@pytest.mark.parametrize("dialect", [0, 1])
def test_predict_large_rotation_increments(dialect):
    """rotation increments on both sides of the 0.5 rad switch between the polynomial and the library sin/cos
    (|w| dt / 2 from 0.05 to 1.5 rad: fast tumbling / long gaps between IMU samples), mixed inside one wave"""
    B = 256
    prm, nom, rot, P, prev = state_batch(B, dialect, 18)
    acc, gyr = imu_of(0, B, 0, 1, nom)
    rng = np.random.default_rng(5)
    axis = rng.normal(size=(B, 3)); axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    half_angle = rng.uniform(0.05, 1.5, B)
    dt = r32(rng.uniform(0.02, 0.2, B))
    gyr0 = r32(axis * (2 * half_angle / dt)[:, None] + nom[:, 13:16])
    with BatchedFilter(B, prm) as flt:
        eng = OracleEngine(B, dialect, 18)
        flt.set_state(nom, rot, P, prev)
        eng.set_state(nom, rot, P, prev)
        flt.predict(acc[0], gyr0, dt)
        eng.predict(acc[0], gyr0, dt)
        _check(flt, eng, 32, "predict, large rotation increments")


@pytest.mark.parametrize("dtype", [32, 64])
@pytest.mark.parametrize("n", [18, 15])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("dialect", [0, 1])
def test_correct_single_step(dialect, mode, n, dtype):
    B, M = 256, 4
    prm, nom, rot, P, prev = state_batch(B, dialect, n)
    ids, pos, quat = markers_of(0, B, 0, M, nom, prm)
    rng = np.random.default_rng(5)
    pos = r32(pos + rng.normal(0, 0.02, pos.shape))      # non-trivial innovations
    ids[0] = -1                                           # nothing visible
    ids[1] = [9, -1, 9, -1]                               # only an id outside the map
    ids[2, 1] = -1
    ids[3, 0] = 9
    prev = rng.choice([0, 1, 2, 16], B).astype(np.int32)
    with BatchedFilter(B, prm, dtype=dtype, nstate=n) as flt:
        eng = OracleEngine(B, dialect, n)
        flt.set_state(nom, rot, P, prev)
        eng.set_state(nom, rot, P, prev)
        flt.correct(ids, pos, quat, mode)
        ok = eng.correct(ids, pos, quat, mode)
        assert (flt.applied() == ok).all()
        assert ok[0] == 0 and ok[1] == 0 and ok[4:].all()
        _check(flt, eng, dtype, f"correct mode {mode}")


@pytest.mark.parametrize("dialect", [0, 1])
def test_golden_vectors(dialect):
    """committed fixtures (tests/golden/ekf_random.npz, numpy twin) through the GPU."""
    g = np.load(os.path.join(GOLD, "ekf_random.npz"))
    for n in (18, 15):
        t = f"d{dialect}_n{n}"
        B = g[t + "_nom"].shape[0]
        with BatchedFilter(B, params_of(dialect), dtype=32, nstate=n) as flt:
            flt.set_state(g[t + "_nom"], g[t + "_rot"], g[t + "_P"], g[t + "_prev"])
            flt.predict(g[t + "_acc"], g[t + "_gyr"], g[t + "_dt"])
            nom, rot, P, _ = flt.get_state()
            sl = slice(1, None) if dialect == 0 else slice(None)   # filter 0: w == 0, reference NaN (guarded here)
            assert state_rel_err(nom[sl], g[t + "_pred_nom"][sl], g[t + "_pred_P"][sl])[0] <= STATE_TOL
            assert state_rel_err_plain(nom[sl], g[t + "_pred_nom"][sl])[0] <= PLAIN_TOL
            assert cov_rel_err(P, g[t + "_pred_P"]) <= COV_TOL
            assert cov_rel_err_blockwise(P, g[t + "_pred_P"]) <= COV_BLOCK_TOL
            assert np.isfinite(nom).all() and np.isfinite(P).all()          # the guard keeps w == 0 finite
            for mode, name in ((0, "near"), (1, "stack")):
                flt.set_state(g[t + "_nom"], g[t + "_rot"], g[t + "_P"], g[t + "_prev"])
                flt.correct(g[t + "_ids"], g[t + "_pos"], g[t + "_quat"], mode)
                nom, rot, P, prev = flt.get_state()
                assert (flt.applied() == g[f"{t}_{name}_ok"]).all()
                assert (prev == g[f"{t}_{name}_prev"]).all()
                assert state_rel_err(nom, g[f"{t}_{name}_nom"], g[f"{t}_{name}_P"])[0] <= STATE_TOL
                assert state_rel_err_plain(nom, g[f"{t}_{name}_nom"])[0] <= PLAIN_TOL
                assert cov_rel_err(P, g[f"{t}_{name}_P"]) <= COV_TOL
                assert cov_rel_err_blockwise(P, g[f"{t}_{name}_P"]) <= COV_BLOCK_TOL


# ------------------------------------------------------------------ free-running windows
@pytest.mark.parametrize("dialect", [0, 1])
def test_free_running_100_frames(dialect):
    """200 Hz IMU + 30 Hz stereo pattern (7,7,6 predicts per correct), M = 4, 100 frames."""
    B, M, n = 128, 4, 18
    prm, nom, rot, P, prev = state_batch(B, dialect, n, mixed=False)
    with BatchedFilter(B, prm, dtype=32, nstate=n) as flt:
        eng = OracleEngine(B, dialect, n)
        flt.set_state(nom, rot, P, prev)
        eng.set_state(nom, rot, P, prev)
        step = 0
        worst = (0.0, 0.0)
        for frame in range(100):
            K = (7, 7, 6)[frame % 3]
            acc, gyr = imu_of(0, B, step, K, nom)
            step += K
            for k in range(K):
                flt.predict(acc[k], gyr[k], DT)
                eng.predict(acc[k], gyr[k], DT)
            ids, pos, quat = markers_of(0, B, frame, M, nom, prm)
            mode = 1 if frame % 2 else 0
            flt.correct(ids, pos, quat, mode)
            eng.correct(ids, pos, quat, mode)
            if frame % 10 == 9:
                # free running: both sides carry their own fp32 / fp64 state, so the innovation y - h(x) (|y| ~ 1 m,
                # |y - h| ~ 1e-3 m) differs by the ~1e-7 m the fp32 position has drifted, times gains of ~10 (rad/s)/m
                # on the weakly observed gyro bias: ~1e-6 rad/s absolute on a 2e-3 rad/s bias whose sigma is 0.1 rad/s.
                # The plain per-block figure (relative to |x| alone) is printed and bounded at PLAIN_WINDOW_TOL.
                es, ec = _check(flt, eng, 32, f"frame {frame}", state_tol=WINDOW_TOL, plain_tol=PLAIN_WINDOW_TOL,
                                cov_block_tol=10 * COV_BLOCK_TOL)
                worst = (max(worst[0], es), max(worst[1], ec))
        print(f"free-run dialect {dialect}: worst state {worst[0]:.3g} cov {worst[1]:.3g}")


def test_land_recording_slice_replay():
    """config 1 plumbing on the GPU: the committed land-recording slice through replay()."""
    d = np.load(os.path.join(GOLD, "land_slice.npz"))
    for dialect, key in ((0, "states_matlab"), (1, "states_cpp")):
        prm = params_of(dialect)
        with BatchedFilter(1, prm, dtype=32, nstate=18) as flt:
            states, npred = replay.replay(flt, d["imu"], d["image"], prm, max_frames=len(d[key]))
        assert (npred == d["npredict"]).all()
        gold = d[key]
        Pg = gold[:, 29:].reshape(-1, 18, 18)
        assert state_rel_err_literal(states[:, 1:20], gold[:, 1:20]) <= STATE_TOL
        assert state_rel_err(states[:, 1:20], gold[:, 1:20], Pg)[0] <= WINDOW_TOL   # ~2000 fp32 steps free-running
        assert cov_rel_err(states[:, 29:].reshape(-1, 18, 18), gold[:, 29:].reshape(-1, 18, 18)) <= COV_TOL
        assert cov_rel_err_blockwise(states[:, 29:].reshape(-1, 18, 18), Pg) <= 10 * COV_BLOCK_TOL   # ~2000 steps free-running
        print(f"[parity] land slice replay dialect {dialect}: plain per-block "
              f"{state_rel_err_plain(states[:, 1:20], gold[:, 1:20])[0]:.2e}, cov block-wise "
              f"{cov_rel_err_blockwise(states[:, 29:].reshape(-1, 18, 18), Pg):.2e}")
        with BatchedFilter(1, prm, dtype=64, nstate=18) as flt:
            states, _ = replay.replay(flt, d["imu"], d["image"], prm, max_frames=len(d[key]))
        assert np.abs(states[:, 1:20] - gold[:, 1:20]).max() < 1e-9


# ------------------------------------------------------------------ algebraic properties on the device
def test_predict_n_equals_repeated_predict():
    B, K = 192, 5
    prm, nom, rot, P, prev = state_batch(B, 0, 18)
    acc, gyr = imu_of(0, B, 0, K, nom)
    dt = np.full(K, DT[0])
    with BatchedFilter(B, prm) as a, BatchedFilter(B, prm) as b:
        a.set_state(nom, rot, P, prev)
        b.set_state(nom, rot, P, prev)
        a.predict_n(acc, gyr, dt)
        for k in range(K):
            b.predict(acc[k], gyr[k], dt[k:k + 1])
        sa, sb = a.get_state(), b.get_state()
        assert state_rel_err(sa[0], sb[0], sa[2])[0] < 2e-6
        assert cov_rel_err(sa[2], sb[2]) < 2e-6 and cov_rel_err_blockwise(sa[2], sb[2]) < 5e-6


@pytest.mark.parametrize("dialect", [0, 1])
def test_joseph_form_equals_simple_form(dialect):
    B, M = 128, 4
    prm, nom, rot, P, prev = state_batch(B, dialect, 18)
    ids, pos, quat = markers_of(0, B, 0, M, nom, prm)
    with BatchedFilter(B, params_of(dialect, 0), dtype=64) as a, BatchedFilter(B, params_of(dialect, 1), dtype=64) as b:
        for f in (a, b):
            f.set_state(nom, rot, P, prev)
            f.correct(ids, pos, quat, 1)
        sa, sb = a.get_state(), b.get_state()
        assert state_rel_err(sa[0], sb[0], sa[2])[0] < 1e-10          # algebraic identity, fp64 kernels
        assert cov_rel_err(sa[2], sb[2]) < 1e-10 and cov_rel_err_blockwise(sa[2], sb[2]) < 1e-10
    with BatchedFilter(B, params_of(dialect, 1)) as b:
        b.set_state(nom, rot, P, prev)
        b.correct(ids, pos, quat, 1)
        eng = OracleEngine(B, dialect, 18, cov_form=1)
        eng.set_state(nom, rot, P, prev)
        eng.correct(ids, pos, quat, 1)
        _check(b, eng, 32, "joseph")


def test_one_stacked_marker_is_the_nearest_marker_update():
    B = 128
    prm, nom, rot, P, prev = state_batch(B, 1, 18)
    ids, pos, quat = markers_of(0, B, 0, 1, nom, prm)
    prev = ids[:, 0].copy()
    with BatchedFilter(B, prm) as a, BatchedFilter(B, prm) as b:
        a.set_state(nom, rot, P, prev)
        b.set_state(nom, rot, P, prev)
        a.correct(ids, pos, quat, 0)
        b.correct(ids, pos, quat, 1)
        sa, sb = a.get_state(), b.get_state()
        # nearest applies the 7 rows one by one, stacked folds them into the 6x6 information matrix first: the same
        # posterior, not the same rounding
        assert state_rel_err(sa[0], sb[0], sb[2], nom)[0] < STATE_TOL
        assert cov_rel_err(sa[2], sb[2]) < COV_TOL and cov_rel_err_blockwise(sa[2], sb[2]) < COV_BLOCK_TOL


@pytest.mark.parametrize("dialect", [0, 1])
def test_n15_is_n18_without_gravity_uncertainty(dialect):
    B, M = 128, 4
    prm, nom, rot, P15, prev = state_batch(B, dialect, 15)
    P18 = np.zeros((B, 18, 18))
    P18[:, :15, :15] = P15
    acc, gyr = imu_of(0, B, 0, 3, nom)
    ids, pos, quat = markers_of(0, B, 0, M, nom, prm)
    for dtype, tol in ((64, 1e-10), (32, STATE_TOL)):
        with BatchedFilter(B, prm, nstate=15, dtype=dtype) as a, BatchedFilter(B, prm, nstate=18, dtype=dtype) as b:
            a.set_state(nom, rot, P15, prev)
            b.set_state(nom, rot, P18, prev)
            for f in (a, b):
                for k in range(3):
                    f.predict(acc[k], gyr[k], DT)
                f.correct(ids, pos, quat, 1)
            sa, sb = a.get_state(), b.get_state()
            assert state_rel_err(sa[0], sb[0], sa[2])[0] < tol
            assert cov_rel_err(sa[2], sb[2][:, :15, :15]) < tol
            assert cov_rel_err_blockwise(sa[2], sb[2][:, :15, :15]) < tol
            assert np.abs(sb[2][:, 15:, :]).max() == 0


def test_skip_mask_and_state_roundtrip():
    B, M = 100, 2
    prm, nom, rot, P, prev = state_batch(B, 0, 18)
    ids, pos, quat = markers_of(0, B, 0, M, nom, prm)
    skip = (np.arange(B) % 3 == 0).astype(np.uint8)
    with BatchedFilter(B, prm, dtype=64) as flt:
        flt.set_state(nom, rot, P, prev)
        s0 = flt.get_state()
        assert np.array_equal(s0[0], nom) and np.array_equal(s0[1], rot) and np.array_equal(s0[3], prev)
        assert np.abs(s0[2] - P).max() < 1e-18
        flt.correct(ids, pos, quat, 0, skip)
        s1 = flt.get_state()
        ap = flt.applied()
        assert (ap == (1 - skip)).all()
        assert np.array_equal(s1[0][skip == 1], nom[skip == 1])
        assert not np.array_equal(s1[0][skip == 0], nom[skip == 0])
        flt.reset_cov()
        P0 = flt.get_state()[2]
        assert np.allclose(P0, np.diag(np.repeat(np.array(list(prm.p0_diag)), 3))[None])


@pytest.mark.parametrize("dialect", [0, 1])
def test_nearest_marker_among_many_slots(dialect):
    """reference mode with more slots than one fetch group (12 markers spread over 16 slots): the nearest-marker scan
    runs over four groups; in the C++ dialect the previously used marker sits in a late group (hysteresis,
    filter.cpp:652-664) for half of the filters"""
    B = 96                                          # not a multiple of 64: a ragged last tile
    prm, nom, rot, P, prev = state_batch(B, dialect, 18)
    ids, pos, quat = markers_of(0, B, 3, 12, nom, prm)
    ids16 = np.full((B, 16), -1, np.int32); ids16[:, [0, 1, 2, 4, 5, 7, 8, 9, 11, 12, 14, 15]] = ids
    pos16 = np.zeros((B, 16, 3)); quat16 = np.zeros((B, 16, 4)); quat16[:, :, 0] = 1
    pos16[:, [0, 1, 2, 4, 5, 7, 8, 9, 11, 12, 14, 15]] = pos
    quat16[:, [0, 1, 2, 4, 5, 7, 8, 9, 11, 12, 14, 15]] = quat
    prev = np.where(np.arange(B) % 2 == 0, ids16[:, 14], prev).astype(np.int32)
    for dtype in (32, 64):
        with BatchedFilter(B, prm, dtype=dtype) as flt:
            eng = OracleEngine(B, dialect, 18)
            flt.set_state(nom, rot, P, prev)
            eng.set_state(nom, rot, P, prev)
            flt.correct(ids16, pos16, quat16, 0)
            ok = eng.correct(ids16, pos16, quat16, 0)
            assert (flt.applied() == ok).all() and ok.all()
            _check(flt, eng, dtype, f"nearest of 16 slots, dialect {dialect}")


@pytest.mark.parametrize("mode", [0, 1])
def test_skip_mask_ragged_batch_and_invisible_markers(mode):
    """lanes that are skipped, lanes past the batch end and filters without any visible marker run through the same
    prologue as live lanes: nothing of theirs may be written"""
    B, M = 100, 4
    prm, nom, rot, P, prev = state_batch(B, 1, 18)
    ids, pos, quat = markers_of(0, B, 1, M, nom, prm)
    ids = ids.copy()
    ids[5::10] = -1                                 # no visible marker at all
    ids[3::10, 1:] = -1                             # one visible marker
    ids[7::10, 0] = 999                             # an id that is not in the map (dropped; others still apply)
    skip = (np.arange(B) % 4 == 1).astype(np.uint8)
    with BatchedFilter(B, prm) as flt:
        eng = OracleEngine(B, 1, 18)
        flt.set_state(nom, rot, P, prev)
        eng.set_state(nom, rot, P, prev)
        flt.correct(ids, pos, quat, mode, skip)
        keep = [x.copy() for x in eng.get_state()]
        ok = eng.correct(ids, pos, quat, mode)
        now = eng.get_state()
        for x, y in zip(now, keep):
            x[skip == 1] = y[skip == 1]
        eng.set_state(*now)
        ok[skip == 1] = 0
        assert (flt.applied() == ok).all()
        assert not ok[5::10].any()
        _check(flt, eng, 32, f"skip + ragged, mode {mode}")
        got = flt.get_state()
        untouched = (ok == 0)
        assert np.array_equal(got[0][untouched], nom[untouched].astype(np.float32).astype(np.float64))


# ------------------------------------------------------------------ full size (BASELINE.json batch)
def test_full_batch_properties_and_shard_equality():
    """B = 65 536 (the headline batch): size-independent properties instead of an oracle run --
    unit quaternions, exactly symmetric and positive definite covariances on a sample, an oracle
    spot check on a strided subset, and sharded == unsharded bit for bit."""
    import torch
    B, M, n = 65536, 4, 18
    prm = params_of(0)
    nom, rot, P, prev = synth.initial_state(0, B, list(prm.p0_diag), n)
    nom, rot, P = r32(nom), r32(rot), r32(P)
    acc, gyr = imu_of(0, B, 0, 3, nom)
    ids, pos, quat = markers_of(0, B, 0, M, nom, prm)
    dev = torch.device("cuda:0")
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    d_acc, d_gyr, d_dt = f32(acc), f32(gyr), f32(np.full(3, DT[0]))
    d_ids, d_pos, d_quat = torch.from_numpy(ids).to(dev), f32(pos), f32(quat)

    def run(lo, hi):
        with BatchedFilter(hi - lo, prm) as flt:
            flt.set_state(nom[lo:hi], rot[lo:hi], P[lo:hi], prev[lo:hi])
            flt.frame(d_acc[:, lo:hi].contiguous(), d_gyr[:, lo:hi].contiguous(), d_dt,
                      d_ids[lo:hi].contiguous(), d_pos[lo:hi].contiguous(), d_quat[lo:hi].contiguous(), 1)
            flt.sync()
            return flt.get_state()

    full = run(0, B)
    assert np.isfinite(full[0]).all() and np.isfinite(full[2]).all()
    assert np.abs(np.linalg.norm(full[0][:, 6:10], axis=1) - 1).max() < 1e-6
    assert np.abs(full[2] - np.swapaxes(full[2], 1, 2)).max() == 0
    sample = full[2][::997].astype(np.float64)
    assert np.linalg.eigvalsh(sample).min() > 0
    halves = [run(0, B // 2), run(B // 2, B)]
    for k in range(4):
        assert np.array_equal(np.concatenate([halves[0][k], halves[1][k]]), full[k])
    sub = np.arange(0, B, 509)
    eng = OracleEngine(len(sub), 0, n)
    eng.set_state(nom[sub], rot[sub], P[sub], prev[sub])
    for k in range(3):
        eng.predict(acc[k][sub], gyr[k][sub], DT)
    eng.correct(ids[sub], pos[sub], quat[sub], 1)
    assert state_rel_err(full[0][sub], eng.nominal, eng.P)[0] <= STATE_TOL
    assert cov_rel_err(full[2][sub], eng.P) <= COV_TOL
    assert cov_rel_err_blockwise(full[2][sub], eng.P) <= COV_BLOCK_TOL
    assert state_rel_err_plain(full[0][sub], eng.nominal)[0] <= PLAIN_TOL


@pytest.mark.parametrize("dialect", [0, 1])
@pytest.mark.parametrize("n", [18, 15])
def test_row_split_correct_of_large_launches(dialect, n):
    """fp32 stacked correct from 2048 waves on (B >= 131 072) runs as the row-split instantiation (two waves per SIMD,
    kernels_tu.hip): parity with the oracle on a strided subset, and the same posterior as the one-wave kernel that the two
    half batches get (different evaluation order of the same six rank-1 passes, so fp32-close, not bit-equal)."""
    B, M = 131072, 4
    prm = params_of(dialect)
    nom, rot, P, prev = synth.initial_state(0, B, list(prm.p0_diag), n)
    nom, rot, P = r32(nom), r32(rot), r32(P)
    ids, pos, quat = markers_of(0, B, 0, M, nom, prm)
    ids[5] = -1
    ids[70, 1:] = -1

    def run(lo, hi):
        with BatchedFilter(hi - lo, prm, nstate=n) as flt:
            flt.set_state(nom[lo:hi], rot[lo:hi], P[lo:hi], prev[lo:hi])
            flt.correct(ids[lo:hi], pos[lo:hi], quat[lo:hi], 1)
            return flt.get_state(), np.asarray(flt.applied())

    full, app = run(0, B)
    halves = [run(0, B // 2), run(B // 2, B)]
    assert np.array_equal(app, np.concatenate([h[1] for h in halves])) and app[5] == 0 and app[70] == 1
    sub = np.unique(np.concatenate([np.arange(0, B, 1021), [5, 70, B - 1]]))
    eng = OracleEngine(len(sub), dialect, n)
    eng.set_state(nom[sub], rot[sub], P[sub], prev[sub])
    eng.correct(ids[sub], pos[sub], quat[sub], 1)
    assert_parity([a[sub] for a in full], eng.get_state(), 32, f"row-split correct d{dialect} n{n}")
    one_wave = [np.concatenate([halves[0][0][k], halves[1][0][k]]) for k in range(4)]
    e = parity_errors(full, one_wave)
    print(f"[split vs one-wave kernel] sigma {e['sigma']:.2e} plain {e['plain']:.2e} cov block {e['cov_block']:.2e}")
    assert e["sigma"] <= STATE_TOL and e["plain"] <= PLAIN_TOL and e["cov_block"] <= COV_BLOCK_TOL and e["asym"] == 0
    assert np.abs(full[2] - np.swapaxes(full[2], 1, 2)).max() == 0


@pytest.mark.parametrize("dialect", [0, 1])
@pytest.mark.parametrize("n", [18, 15])
def test_two_wave_frame_and_predict_n_of_large_launches(dialect, n):
    """from 2048 waves on the fused frame (stacked) and predict_n run as the 256-register kernels (frame2_kernel, parked
    predict loop: rows p and part of the nominal state wait in LDS between their uses): parity with the oracle on a strided
    subset and fp32-closeness to the one-wave kernels that the two half batches get"""
    import torch
    B, M, K = 131072, 4, 5
    prm = params_of(dialect)
    nom, rot, P, prev = synth.initial_state(0, B, list(prm.p0_diag), n)
    nom, rot, P = r32(nom), r32(rot), r32(P)
    acc, gyr = imu_of(0, B, 0, K, nom)
    ids, pos, quat = markers_of(0, B, 0, M, nom, prm)
    ids[5] = -1                                                 # a filter that sees nothing: predicted record only
    skip = np.zeros(B, np.uint8); skip[9] = 1                   # ... and one whose camera frame is masked
    dev = torch.device("cuda:0")
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    d_acc, d_gyr, d_dt = f32(acc), f32(gyr), f32(np.full(K, DT[0]))
    d_ids, d_pos, d_quat, d_skip = torch.from_numpy(ids).to(dev), f32(pos), f32(quat), torch.from_numpy(skip).to(dev)

    def run(lo, hi, what):
        with BatchedFilter(hi - lo, prm, nstate=n) as flt:
            flt.set_state(nom[lo:hi], rot[lo:hi], P[lo:hi], prev[lo:hi])
            a, g = d_acc[:, lo:hi].contiguous(), d_gyr[:, lo:hi].contiguous()
            if what == "frame":
                flt.frame(a, g, d_dt, d_ids[lo:hi].contiguous(), d_pos[lo:hi].contiguous(), d_quat[lo:hi].contiguous(), 1,
                          skip=d_skip[lo:hi].contiguous(), fused=True)
            else:
                flt.predict_n(a, g, d_dt, K)
            flt.sync()
            return flt.get_state(), (np.asarray(flt.applied()) if what == "frame" else None)

    sub = np.unique(np.concatenate([np.arange(0, B, 1021), [5, 9, B - 1]]))
    for what in ("predict_n", "frame"):
        full, app = run(0, B, what)
        halves = [run(0, B // 2, what), run(B // 2, B, what)]
        eng = OracleEngine(len(sub), dialect, n)
        eng.set_state(nom[sub], rot[sub], P[sub], prev[sub])
        for k in range(K):
            eng.predict(acc[k][sub], gyr[k][sub], DT)
        if what == "frame":
            assert np.array_equal(app, np.concatenate([h[1] for h in halves])) and app[5] == 0 and app[9] == 0 and app[0] == 1
            ids_o = ids.copy(); ids_o[skip == 1] = -1           # a masked frame is a frame without markers
            eng.correct(ids_o[sub], pos[sub], quat[sub], 1)
        # a window of K + 1 fp32 steps: the window bound, as in the fused-frame and free-running tests
        assert_parity([a[sub] for a in full], eng.get_state(), 32, f"two-wave {what} d{dialect} n{n}", state_tol=WINDOW_TOL,
                      plain_tol=PLAIN_WINDOW_TOL)
        one_wave = [np.concatenate([halves[0][0][k], halves[1][0][k]]) for k in range(4)]
        e = parity_errors(full, one_wave)
        print(f"[two-wave vs one-wave {what}] sigma {e['sigma']:.2e} plain {e['plain']:.2e} cov block {e['cov_block']:.2e}")
        assert e["sigma"] <= STATE_TOL and e["plain"] <= PLAIN_TOL and e["cov_block"] <= COV_BLOCK_TOL and e["asym"] == 0


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("dialect", [0, 1])
def test_frame_window_equals_a_sequence_of_fused_frames(dialect, mode):
    """fbus_ekf_frames_fused_dev: F frames (K_f predicts + a correct each) in ONE launch with the records resident in
    registers throughout == F fused-frame launches bit for bit (same device functions, same order), and parity with the
    oracle over the window; ragged batch, an invisible marker set, a masked frame, a frame without IMU samples; fp64 and
    the (Joseph, nearest) combination take the frame-by-frame route behind the same entry point."""
    import torch
    B, M = 1000 - 3, 4
    kcount = [7, 0, 6, 3]
    F, Kt = len(kcount), sum(kcount)
    prm, nom, rot, P, prev = state_batch(B, dialect, 18)
    acc, gyr = imu_of(0, B, 0, Kt, nom)
    dev = torch.device("cuda:0")
    frames = [markers_of(0, B, f, M, nom, prm) for f in range(F)]
    ids = np.stack([f[0] for f in frames]); pos = np.stack([f[1] for f in frames]); quat = np.stack([f[2] for f in frames])
    ids[1, 5] = -1
    ids[2, 6, :] = 9
    skip = np.zeros((F, B), np.uint8); skip[2, 11] = 1; skip[3, 12] = 1
    for dtype, joseph in ((32, False), (32, True), (64, False)):
        prm.cov_form = capi.COV_JOSEPH if joseph else capi.COV_SIMPLE
        tt = torch.float32 if dtype == 32 else torch.float64
        dd = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev).to(tt)
        d_acc, d_gyr, d_dt = dd(acc), dd(gyr), dd(np.full(Kt, DT[0]))
        d_ids, d_pos, d_quat, d_skip = torch.from_numpy(ids).to(dev), dd(pos), dd(quat), torch.from_numpy(skip).to(dev)
        with BatchedFilter(B, prm, dtype=dtype) as fa, BatchedFilter(B, prm, dtype=dtype) as fb:
            fa.set_state(nom, rot, P, prev); fb.set_state(nom, rot, P, prev)
            fa.frames(kcount, d_acc, d_gyr, d_dt, d_ids, d_pos, d_quat, mode, skip=d_skip)
            k0 = 0
            for f, K in enumerate(kcount):
                fb.frame(d_acc[k0:k0 + K] if K else None, d_gyr[k0:k0 + K] if K else None, d_dt[k0:k0 + K] if K else None,
                         d_ids[f], d_pos[f], d_quat[f], mode, skip=d_skip[f], fused=True)
                k0 += K
            fa.sync(); fb.sync()
            sa, sb = fa.get_state(), fb.get_state()
            assert np.array_equal(fa.applied(), fb.applied())
            for k in range(4):
                assert np.array_equal(sa[k], sb[k]), (dtype, joseph, k)
            if joseph:
                continue
            eng = OracleEngine(B, dialect, 18)
            eng.set_state(nom, rot, P, prev)
            k0 = 0
            for f, K in enumerate(kcount):
                for k in range(K):
                    eng.predict(acc[k0 + k], gyr[k0 + k], DT)
                k0 += K
                ids_f = ids[f].copy(); ids_f[skip[f] == 1] = -1
                eng.correct(ids_f, pos[f], quat[f], mode)
            # a window of 16 predicts and 4 corrects: the window bounds (the single-step 1e-5 is asserted step by step elsewhere)
            e = parity_errors(sa, eng.get_state())
            print(f"[parity] frame window d{dialect} mode {mode} fp{dtype}: literal {e['literal']:.2e} sigma-aware {e['sigma']:.2e} "
                  f"plain {e['plain']:.2e} cov {e['cov']:.2e} cov block-wise {e['cov_block']:.2e}")
            if dtype == 64:
                assert max(e["literal"], e["sigma"], e["plain"], e["cov"]) <= 1e-9 and e["cov_block"] <= 1e-11
            else:
                # tests/util.py's window gate: literal 1e-5 (C++ dialect, N = 18: the stated 3e-5 -- util.py); here the block-wise
                # covariance even meets its single-step bound
                assert_window_parity(sa, eng.get_state(), f"frame window d{dialect} mode {mode} fp32 (gate)", dialect, 18, verbose=False)
                assert e["cov_block"] <= COV_BLOCK_TOL
            assert e["asym"] == 0 and e["prev_equal"]
    prm.cov_form = capi.COV_SIMPLE


def test_two_wave_kernels_on_small_and_ragged_batches():
    """The launchers pick the 256-register kernels (row-split correct, parked predict_n, frame2_kernel) from 2048 waves on.
    With FBUS_TWO_WAVE_MIN_B=0 (read once per process, hence the child pytest) they take every launch, so the tests written
    for partial tiles, skip masks, invisible markers, 16 marker slots, graph replay and long runs exercise THEM."""
    import subprocess
    import sys
    if os.environ.get("FBUS_TWO_WAVE_MIN_B") == "0":
        pytest.skip("already inside the forced run")
    env = dict(os.environ, FBUS_TWO_WAVE_MIN_B="0")
    sel = ("fused_frame or skip_mask or predict_n_equals or sixteen_marker or one_stacked or graph_replay or long_run or "
           "correct_single_step or free_running")
    sel = f"({sel}) and not frame_window"       # that test asserts bit-equality of two kernels of the SAME (one-wave) family
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-k", sel],
                       env=env, capture_output=True, text=True, timeout=1500)
    tail = r.stdout[-1500:]
    assert r.returncode == 0 and " passed" in tail and "failed" not in tail, tail


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("dialect", [0, 1])
def test_fused_frame_equals_per_call_launches(dialect, mode):
    """one launch per frame (records resident in registers) vs K predict launches + one correct launch"""
    import torch
    B, M, K = 1000, 4, 7
    prm, nom, rot, P, prev = state_batch(B, dialect, 18)
    acc, gyr = imu_of(0, B, 0, 2 * K, nom)
    dev = torch.device("cuda:0")
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    d_acc, d_gyr, d_dt = f32(acc), f32(gyr), f32(np.full(K, DT[0]))
    frames = []
    for f in range(2):
        ids, pos, quat = markers_of(0, B, f, M, nom, prm)
        ids[5] = -1
        ids[6, :] = 9
        frames.append((torch.from_numpy(ids).to(dev), f32(pos), f32(quat)))
    skip = torch.from_numpy((np.arange(B) % 7 == 3).astype(np.uint8)).to(dev)
    with BatchedFilter(B, prm) as a, BatchedFilter(B, prm) as b:
        for flt, fused in ((a, False), (b, True)):
            flt.set_state(nom, rot, P, prev)
            for f in range(2):
                ids, pos, quat = frames[f]
                flt.frame(d_acc[f * K:(f + 1) * K], d_gyr[f * K:(f + 1) * K], d_dt, ids, pos, quat, mode,
                          skip if f == 1 else None, fused=fused)
            flt.sync()
        sa, sb = a.get_state(), b.get_state()
        assert (a.applied() == b.applied()).all()
        assert (sa[3] == sb[3]).all()
        # same device functions, but two separately compiled kernels: fp contraction / association may differ,
        # so the two fp32 results agree to rounding (compounded over 16 steps), not bit for bit
        assert state_rel_err(sb[0], sa[0], sa[2])[0] < WINDOW_TOL and cov_rel_err(sb[2], sa[2]) < 1e-5
        assert cov_rel_err_blockwise(sb[2], sa[2]) < COV_BLOCK_TOL
        eng = OracleEngine(B, dialect, 18)
        eng.set_state(nom, rot, P, prev)
        skip_h = skip.cpu().numpy()
        for f in range(2):
            for k in range(K):
                eng.predict(acc[f * K + k], gyr[f * K + k], DT)
            ids_h, pos_h, quat_h = frames[f][0].cpu().numpy(), frames[f][1].cpu().numpy().astype(np.float64), frames[f][2].cpu().numpy().astype(np.float64)
            keep = eng.get_state()
            ok = eng.correct(ids_h, pos_h, quat_h, mode)
            if f == 1:                                    # emulate the skip mask on the oracle side
                now = eng.get_state()
                for x, y in zip(now[:3], keep[:3]):
                    x[skip_h == 1] = y[skip_h == 1]
                now[3][skip_h == 1] = keep[3][skip_h == 1]
                eng.set_state(*now)
                ok[skip_h == 1] = 0
        assert (b.applied() == ok).all()
        assert state_rel_err(sb[0], eng.nominal, eng.P)[0] < WINDOW_TOL and cov_rel_err(sb[2], eng.P) < COV_TOL
        assert cov_rel_err_blockwise(sb[2], eng.P) < COV_BLOCK_TOL
        print(f"[parity] fused frame dialect {dialect} mode {mode}: plain per-block "
              f"{state_rel_err_plain(sb[0], eng.nominal)[0]:.2e}, cov block-wise {cov_rel_err_blockwise(sb[2], eng.P):.2e}")
        # predicts only (M = 0) through the fused entry point
        b.set_state(nom, rot, P, prev)
        a.set_state(nom, rot, P, prev)
        b.frame(d_acc[:K], d_gyr[:K], d_dt, None, None, None, mode, fused=True)
        a.predict_n(d_acc[:K], d_gyr[:K], d_dt)
        a.sync(); b.sync()
        sa, sb = a.get_state(), b.get_state()
        assert state_rel_err(sb[0], sa[0], sa[2])[0] < STATE_TOL and cov_rel_err(sb[2], sa[2]) < 1e-5
        assert cov_rel_err_blockwise(sb[2], sa[2]) < COV_BLOCK_TOL


@pytest.mark.parametrize("n", [18, 15])
@pytest.mark.parametrize("dialect", [0, 1])
def test_fp64_resident_frame_and_predict_n(dialect, n):
    """(round 4) the reference's own arithmetic as ONE launch per camera frame and one launch per K IMU samples: frame2_kernel<double>
    (parked K-step predict loop + row-split passes) and the parked predict_n<double>, against the oracle at the fp64 gates (1e-9) and
    against the per-call fp64 kernels, over two frames with invisible markers, ids outside the map and a masked frame.
    Types of the reference: common.hpp:205-247; operations: filter.cpp:533-616, 622-741."""
    import torch
    B, M, K = 1000, 4, 7
    prm, nom, rot, P, prev = state_batch(B, dialect, n)
    acc, gyr = imu_of(0, B, 0, 2 * K, nom)
    dev = torch.device("cuda:0")
    f64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(dev)
    d_acc, d_gyr, d_dt = f64(acc), f64(gyr), f64(np.full(K, DT[0]))
    frames = []
    for f in range(2):
        ids, pos, quat = markers_of(0, B, f, M, nom, prm)
        ids[5] = -1
        ids[6, :] = 9
        frames.append((torch.from_numpy(ids).to(dev), f64(pos), f64(quat)))
    skip = torch.from_numpy((np.arange(B) % 7 == 3).astype(np.uint8)).to(dev)
    with BatchedFilter(B, prm, dtype=64, nstate=n) as a, BatchedFilter(B, prm, dtype=64, nstate=n) as b:
        for flt, fused in ((a, False), (b, True)):
            flt.set_state(nom, rot, P, prev)
            for f in range(2):
                ids, pos, quat = frames[f]
                flt.frame(d_acc[f * K:(f + 1) * K], d_gyr[f * K:(f + 1) * K], d_dt, ids, pos, quat, 1, skip if f == 1 else None, fused=fused)
            flt.sync()
        sa, sb = a.get_state(), b.get_state()
        assert (a.applied() == b.applied()).all() and (sa[3] == sb[3]).all()
        assert_parity(sb, sa, 64, f"fp64 resident frame vs per-call launches d{dialect} n{n}")
        eng = OracleEngine(B, dialect, n)
        eng.set_state(nom, rot, P, prev)
        skip_h = skip.cpu().numpy()
        for f in range(2):
            for k in range(K):
                eng.predict(acc[f * K + k], gyr[f * K + k], DT)
            keep = eng.get_state()
            ok = eng.correct(frames[f][0].cpu().numpy(), frames[f][1].cpu().numpy(), frames[f][2].cpu().numpy(), 1)
            if f == 1:
                now = eng.get_state()
                for x, y in zip(now[:3], keep[:3]):
                    x[skip_h == 1] = y[skip_h == 1]
                now[3][skip_h == 1] = keep[3][skip_h == 1]
                eng.set_state(*now)
                ok[skip_h == 1] = 0
        assert (b.applied() == ok).all()
        assert_parity(sb, eng.get_state(), 64, f"fp64 resident frame vs oracle d{dialect} n{n}")
        # K steps in one launch against K launches, and a frame without markers through the fused entry point
        a.set_state(nom, rot, P, prev); b.set_state(nom, rot, P, prev)
        for k in range(K):
            a.predict(d_acc[k], d_gyr[k], d_dt[:1])
        b.predict_n(d_acc[:K], d_gyr[:K], d_dt)
        a.sync(); b.sync()
        assert_parity(b.get_state(), a.get_state(), 64, f"fp64 resident predict_n vs per-call d{dialect} n{n}")
        b.set_state(nom, rot, P, prev)
        b.frame(d_acc[:K], d_gyr[:K], d_dt, None, None, None, 1, fused=True)
        b.sync()
        assert_parity(b.get_state(), a.get_state(), 64, f"fp64 resident frame without markers d{dialect} n{n}")


def test_sixteen_marker_slots_stacked():
    """config 5 shape: M = 16 slots per frame (12 distinct map markers + 4 absent), stacked 84-row update"""
    B = 192
    prm, nom, rot, P, prev = state_batch(B, 0, 18)
    ids, pos, quat = markers_of(0, B, 0, 12, nom, prm)
    ids16 = np.full((B, 16), -1, np.int32); ids16[:, 2:14] = ids
    pos16 = np.zeros((B, 16, 3)); pos16[:, 2:14] = pos
    quat16 = np.zeros((B, 16, 4)); quat16[:, :, 0] = 1; quat16[:, 2:14] = quat
    for dtype in (32, 64):
        with BatchedFilter(B, prm, dtype=dtype) as flt:
            eng = OracleEngine(B, 0, 18)
            flt.set_state(nom, rot, P, prev)
            eng.set_state(nom, rot, P, prev)
            flt.correct(ids16, pos16, quat16, 1)
            ok = eng.correct(ids16, pos16, quat16, 1)
            assert ok.all() and (flt.applied() == 1).all()
            _check(flt, eng, dtype, "16 slots stacked")    # 84 rows at one linearisation point: the standard gate (round 6; measured 4.2e-7, rounds 2-5 allowed 3x)


def test_long_run_stability_and_degenerate_inputs():
    """10 s of simulated time at B = 4096 through the fused frame kernel: the filters stay finite, the covariance
    stays symmetric positive definite and the quaternion unit; then the degenerate inputs the reference mishandles
    (w == 0 and a zero correction, which are 0/0 in both reference dialects) leave the state finite."""
    import torch
    B, M = 4096, 4
    prm = params_of(0)
    nom, rot, P, prev = synth.initial_state(0, B, list(prm.p0_diag), 18)
    dev = torch.device("cuda:0")
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    with BatchedFilter(B, prm) as flt:
        flt.set_state(nom, rot, P, prev)
        step = 0
        d_dt = f32(np.full(7, DT[0]))
        for frame in range(300):
            K = (7, 7, 6)[frame % 3]
            acc, gyr = synth.imu_samples(0, B, step, K, nom)
            step += K
            ids, pos, quat = synth.marker_frame(0, B, frame, M, nom, prm)
            flt.frame(f32(acc), f32(gyr), d_dt[:K], torch.from_numpy(ids).to(dev), f32(pos), f32(quat), 1, fused=True)
        flt.sync()
        g_nom, _, g_P, _ = flt.get_state()
        assert np.isfinite(g_nom).all() and np.isfinite(g_P).all()
        assert np.abs(np.linalg.norm(g_nom[:, 6:10], axis=1) - 1).max() < 1e-6
        assert np.linalg.eigvalsh(g_P[::37].astype(np.float64)).min() > 0
        assert np.abs(g_nom[:, 0:3] - nom[:, 0:3]).max() < 0.05          # held at the measured pose
        assert np.abs(g_nom[:, 16:19] - [9.8, 0, 0]).max() < 0.5           # gravity estimate converged near truth
        # degenerate inputs: gyro == gyro bias (w == 0) and a measurement equal to the prediction
        # (per-call predict, Matlab dialect, finiteness only: tests/test_imu_edges_gpu.py holds these and the other edges of predict's
        # domain against the oracle on every route that predicts, in both dialects)
        flt.set_state(nom, rot, P, prev)
        acc, _ = synth.imu_samples(0, B, 0, 1, nom)
        flt.predict(acc[0], nom[:, 13:16].astype(np.float32).astype(np.float64), DT)
        s = flt.get_state()
        assert np.isfinite(s[0]).all() and np.isfinite(s[2]).all()
        assert np.abs(s[0][:, 6:10] - nom[:, 6:10]).max() < 1e-6           # identity rotation, not NaN
        # ... and a rate whose SQUARE is an fp32 denormal (|w| between 4e-23 and 1.1e-19): v_rsq_f32 returns +inf for it and the
        # Newton step behind it NaN -- the kernels test against the smallest normal number, not against 0 (round-3 advisor finding)
        bias = nom[:, 13:16].astype(np.float32).astype(np.float64)
        nz = nom.copy(); nz[:, 13:16] = 0.0
        for w in (3e-20, 1e-21, 5e-23):
            flt.set_state(nz, rot, P, prev)
            flt.predict(acc[0], np.full((B, 3), w), DT)
            s = flt.get_state()
            assert np.isfinite(s[0]).all() and np.isfinite(s[2]).all(), w
            assert np.abs(s[0][:, 6:10] - nz[:, 6:10]).max() < 1e-6


def test_device_state_io_records_aliasing_and_checkpoint_resume():
    """set/get_state with device arrays, records living in a caller-owned tensor (what the RCCL gather ships),
    and checkpoint -> resume: copying the packed records into a fresh handle continues bit for bit."""
    import torch
    B = 777
    prm, nom, rot, P, prev = state_batch(B, 1, 18)
    prev = (np.arange(B) % 3).astype(np.int32)
    acc, gyr = imu_of(0, B, 0, 4, nom)
    dt = r32(np.random.default_rng(1).uniform(0.002, 0.008, (4, B)))
    dev = torch.device("cuda:0")
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    with BatchedFilter(B, prm) as a, BatchedFilter(B, prm) as b:
        a.set_state(f32(nom), f32(rot), f32(P), torch.from_numpy(prev).to(dev))      # device arrays in
        a.sync()
        s = a.get_state()
        assert np.array_equal(s[0], nom.astype(np.float32)) and np.array_equal(s[3], prev)
        _, bpf, total = a.records()
        assert bpf == 800 and total == 800 * ((B + 63) // 64 * 64)
        rec = torch.empty(total, dtype=torch.uint8, device=dev)
        a.attach_records(rec)
        a.predict_n(acc[:2], gyr[:2], dt[:2])                                          # per-filter dt, host arrays
        snapshot = rec.clone()                                                         # checkpoint
        a.predict_n(acc[2:], gyr[2:], dt[2:])
        ref = a.get_state()
        rec_b = torch.empty(total, dtype=torch.uint8, device=dev)
        b.attach_records(rec_b)
        rec_b.copy_(snapshot)                                                          # resume in another handle
        torch.cuda.synchronize()
        b.predict_n(acc[2:], gyr[2:], dt[2:])
        got = b.get_state()
        assert all(np.array_equal(x, y) for x, y in zip(ref, got))
        eng = OracleEngine(B, 1, 18)
        eng.set_state(nom, rot, P, prev)
        for k in range(4):
            eng.predict(acc[k], gyr[k], dt[k])
        assert state_rel_err(got[0], eng.nominal, eng.P)[0] <= STATE_TOL and cov_rel_err(got[2], eng.P) <= COV_TOL
        assert cov_rel_err_blockwise(got[2], eng.P) <= COV_BLOCK_TOL and state_rel_err_plain(got[0], eng.nominal)[0] <= PLAIN_TOL


def test_hip_graph_replay_equals_eager_launches():
    """a captured frame (7 predict launches + 1 correct launch) replayed from a HIP graph == the eager launches"""
    import torch
    B, M, K = 4096, 4, 7
    prm, nom, rot, P, prev = state_batch(B, 0, 18)
    acc, gyr = imu_of(0, B, 0, K, nom)
    ids, pos, quat = markers_of(0, B, 0, M, nom, prm)
    dev = torch.device("cuda:0")
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    d = [f32(acc), f32(gyr), f32(np.full(K, DT[0])), torch.from_numpy(ids).to(dev), f32(pos), f32(quat)]
    with BatchedFilter(B, prm) as a, BatchedFilter(B, prm) as b:
        a.set_state(nom, rot, P, prev)
        b.set_state(nom, rot, P, prev)
        gid = b.graph_capture(lambda: b.frame(d[0], d[1], d[2], d[3], d[4], d[5], 1))
        untouched = b.get_state()
        assert np.array_equal(untouched[0], nom.astype(np.float32))          # capture records, it does not execute
        for _ in range(3):
            a.frame(d[0], d[1], d[2], d[3], d[4], d[5], 1)
            b.graph_launch(gid)
        a.sync(); b.sync()
        sa, sb = a.get_state(), b.get_state()
        assert all(np.array_equal(x, y) for x, y in zip(sa, sb))
        assert (a.applied() == b.applied()).all()


# ------------------------------------------------------------------ the gate can fail
def test_parity_gate_goes_red_on_a_mutated_result():
    """mutation check of the gate itself: take a green GPU result and damage ONE 3x3 block (or one nominal block) by a
    relative 1e-3 / a factor of two -- every such mutation must turn the gate red.  (The round-1 gate,
    max|dP| / max|P| alone, let a doubled position block pass at 1.3e-6 because P_gg ~ 100 dominates it.)"""
    B, M = 256, 4
    prm, nom, rot, P, prev = state_batch(B, 0, 18)
    acc, gyr = imu_of(0, B, 0, 1, nom)
    ids, pos, quat = markers_of(0, B, 0, M, nom, prm)
    with BatchedFilter(B, prm) as flt:
        eng = OracleEngine(B, 0, 18)
        flt.set_state(nom, rot, P, prev)
        eng.set_state(nom, rot, P, prev)
        flt.predict(acc[0], gyr[0], DT)
        eng.predict(acc[0], gyr[0], DT)
        flt.correct(ids, pos, quat, 1)
        eng.correct(ids, pos, quat, 1)
        got, ref = flt.get_state(), eng.get_state()
    assert_parity(got, ref, 32, "unmutated")
    names = ("p", "v", "theta", "ba", "bg", "g")
    for bi in range(6):
        for bj in range(bi, 6):
            for factor in (2.0, 1.0 + 1e-3, 0.0):
                mut = [x.copy() for x in got]
                blk = mut[2][:, 3 * bi:3 * bi + 3, 3 * bj:3 * bj + 3] * factor
                mut[2][:, 3 * bi:3 * bi + 3, 3 * bj:3 * bj + 3] = blk
                mut[2][:, 3 * bj:3 * bj + 3, 3 * bi:3 * bi + 3] = np.swapaxes(blk, 1, 2)     # keep it symmetric
                if np.array_equal(mut[2], got[2]):
                    continue                                                               # an all-zero block
                with pytest.raises(AssertionError):
                    assert_parity(mut, ref, 32, f"P({names[bi]},{names[bj]}) x {factor}", verbose=False)
    for name, a, b in (("p", 0, 3), ("v", 3, 6), ("q", 6, 10), ("ba", 10, 13), ("bg", 13, 16), ("g", 16, 19)):
        mut = [x.copy() for x in got]
        mut[0][:, a:b] *= 1.0 + 1e-3
        with pytest.raises(AssertionError):
            assert_parity(mut, ref, 32, f"nominal {name} x (1 + 1e-3)", verbose=False)
    mut = [x.copy() for x in got]
    mut[2][:, 0, 1] *= 1.0 + 1e-6                                                          # asymmetry
    with pytest.raises(AssertionError):
        assert_parity(mut, ref, 32, "asymmetric", verbose=False)


def test_frame_entry_points_validate_before_they_launch():
    """a rejected frame call must not leave the state advanced by its K predicts (both entry points check K, M, the pointers
    and the mode up front), and the Python mirror refuses wrongly sized device arrays"""
    import ctypes as C
    import torch
    B, K, M = 256, 3, 2
    prm, nom, rot, P, prev = state_batch(B, 0, 18)
    acc, gyr = imu_of(0, B, 0, K, nom)
    ids, pos, quat = markers_of(0, B, 0, M, nom, prm)
    dev = torch.device("cuda:0")
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    d_acc, d_gyr, d_dt = f32(acc), f32(gyr), f32(np.full(K, DT[0]))
    d_ids, d_pos, d_quat = torch.from_numpy(ids).to(dev), f32(pos), f32(quat)
    p = lambda t: C.c_void_p(t.data_ptr())
    with BatchedFilter(B, prm) as flt:
        flt.set_state(nom, rot, P, prev)
        before = flt.get_state()
        lib, h = flt._lib, flt._h
        for fn in (lib.fbus_ekf_frame_dev, lib.fbus_ekf_frame_fused_dev):
            assert fn(h, K, None, p(d_gyr), p(d_dt), 0, M, p(d_ids), p(d_pos), p(d_quat), 1, None) == 1      # NULL accel
            assert fn(h, K, p(d_acc), p(d_gyr), p(d_dt), 0, 17, p(d_ids), p(d_pos), p(d_quat), 1, None) == 1  # M > FBUS_MAX_VISIBLE
            assert fn(h, K, p(d_acc), p(d_gyr), p(d_dt), 0, M, p(d_ids), None, p(d_quat), 1, None) == 1       # NULL pos
            assert fn(h, K, p(d_acc), p(d_gyr), p(d_dt), 0, M, p(d_ids), p(d_pos), p(d_quat), 7, None) == 4   # unknown mode
            assert fn(h, -1, p(d_acc), p(d_gyr), p(d_dt), 0, M, p(d_ids), p(d_pos), p(d_quat), 1, None) == 1
        # the frame-window entry point: the same checks, plus its frame counts
        fw = lib.fbus_ekf_frames_fused_dev
        kc = lambda *v: (C.c_int32 * len(v))(*v)
        assert fw(h, 1, kc(K), None, p(d_gyr), p(d_dt), 0, M, p(d_ids), p(d_pos), p(d_quat), 1, None) == 1             # NULL accel
        assert fw(h, 1, None, p(d_acc), p(d_gyr), p(d_dt), 0, M, p(d_ids), p(d_pos), p(d_quat), 1, None) == 1          # NULL kcount
        assert fw(h, 65, kc(*([0] * 65)), p(d_acc), p(d_gyr), p(d_dt), 0, M, p(d_ids), p(d_pos), p(d_quat), 1, None) == 1   # too many frames
        assert fw(h, 1, kc(256), p(d_acc), p(d_gyr), p(d_dt), 0, M, p(d_ids), p(d_pos), p(d_quat), 1, None) == 1        # count > 255
        assert fw(h, 1, kc(-1), p(d_acc), p(d_gyr), p(d_dt), 0, M, p(d_ids), p(d_pos), p(d_quat), 1, None) == 1
        assert fw(h, 1, kc(K), p(d_acc), p(d_gyr), p(d_dt), 0, M, p(d_ids), p(d_pos), None, 1, None) == 1              # NULL quat
        assert fw(h, 1, kc(K), p(d_acc), p(d_gyr), p(d_dt), 0, M, p(d_ids), p(d_pos), p(d_quat), 3, None) == 4         # unknown mode
        assert fw(h, 0, None, None, None, None, 0, 0, None, None, None, 1, None) == 0                                   # empty window: nothing to do
        flt.sync()
        after = flt.get_state()
        assert all(np.array_equal(x, y) for x, y in zip(before, after))         # nothing was launched
        with pytest.raises(ValueError):
            flt.frames([K], d_acc, d_gyr[:2], d_dt, d_ids, d_pos, d_quat, 1)      # gyro of the wrong size
        with pytest.raises(ValueError):
            flt.frame(d_acc, d_gyr[:2], d_dt, d_ids, d_pos, d_quat, 1)            # gyro of the wrong size
        with pytest.raises(ValueError):
            flt.frame(d_acc, d_gyr, d_dt, d_ids, d_pos[:, :1], d_quat, 1)         # pos of the wrong size / not contiguous
        flt.frame(d_acc, d_gyr, d_dt, d_ids, d_pos, d_quat, 1)                    # the valid call still works
        flt.sync()
        assert not np.array_equal(flt.get_state()[0], before[0])


def test_streams_are_ordered_by_wait_and_signal():
    """the handle's own stream is non-blocking: inputs produced on torch's stream are ordered in with wait_stream, results are
    handed back with signal_stream, and set_stream(torch stream) shares the stream outright (handle 0 = the legacy default stream)"""
    import torch
    B = 4096
    prm, nom, rot, P, prev = state_batch(B, 0, 18)
    acc, gyr = imu_of(0, B, 0, 1, nom)
    dev = torch.device("cuda:0")
    eng = OracleEngine(B, 0, 18)
    eng.set_state(nom, rot, P, prev)
    eng.predict(acc[0], gyr[0], DT)
    a64 = torch.from_numpy(acc[0]).to(dev); g64 = torch.from_numpy(gyr[0]).to(dev)
    d_dt = torch.full((1,), float(DT[0]), dtype=torch.float32, device=dev)
    for share in (False, True):
        with BatchedFilter(B, prm) as flt:
            flt.set_state(nom, rot, P, prev)
            if share:
                flt.set_stream(torch.cuda.current_stream())           # handle value 0: the legacy default stream
            big = torch.randn(4096, 4096, device=dev)
            for _ in range(4):
                big = big @ big * 1e-3                                # keeps torch's stream busy ahead of the casts
            d_acc, d_gyr = a64.to(torch.float32), g64.to(torch.float32)   # produced on torch's stream, behind the matmuls
            if not share:
                flt.wait_stream(torch.cuda.current_stream())
            flt.predict(d_acc, d_gyr, d_dt)
            if not share:
                flt.signal_stream(torch.cuda.current_stream())
            torch.cuda.current_stream().synchronize()                 # NOT a device-wide sync: only torch's stream
            got = flt.get_state()
        assert state_rel_err(got[0], eng.nominal, eng.P)[0] <= STATE_TOL and cov_rel_err_blockwise(got[2], eng.P) <= COV_BLOCK_TOL
