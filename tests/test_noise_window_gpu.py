"""GPU suite: the resident frame windows with a per-filter noise table (frames_kernel / frame_meas_kernel with (TrajOut, NoiseIn)).

The table of test_noise_gpu.py (G = 5 rows, x0.1 .. x10, round-robin: every wave mixes rows), B = 4197 (a partial last tile) and, on
every handle, set_policy_batch(P) with P = launch_info(INFO_ONE_ROUND_FILTERS): one full round of waves -- above half a chip, so the
tabled handle and its untabled twins both take the one-wave resident forms, and one filter short of INFO_TWO_WAVE_MIN_B, so no
per-call kernel changes to its two-wave form.  Every comparison is bit-equality.

  1 twins      filter b of the tabled window == filter b of an untabled handle whose fbus_params hold row b mod G (records, applied,
               every trajectory row)
  2 route      launch_info(INFO_NOISE_RESIDENT)
  3 frames     the tabled window == the same frames through the tabled single-frame fused entry points
  4 identity   65 536 filters, the handle's own policy batch: a table equal to fbus_params changes nothing
  5 fallbacks  small policy batch / likelihood sums on / (Joseph, nearest): the window == predict_n + the per-call update per frame
  6 graph      a captured resident tabled window reads the table as rewritten in place
  7 sweep      the land recording through replay_windowed: every filter == its untabled twin; the rows' end states differ
"""
import os

import numpy as np
import pytest
import torch

from fbus_ekf import BatchedFilter, capi, noise, replay, synth
from support import (B_ODD, G, assert_twin, handle, imu, perturbed_setup, r32, rows_of, run_twins, same_state, state_of, to_device,
                     with_row)
from util import state_rel_err_literal

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KC = [3, 0, 2, 4, 1]                            # IMU samples in front of each frame: unequal, one frame without any
F = len(KC)
M = 4
F32 = np.float32
_P = []


def policy_p():
    """one full round of waves: the policy batch of every handle here"""
    if not _P:
        with BatchedFilter(64, capi.default_params(0), dtype=32) as f:
            p = f.launch_info(capi.INFO_ONE_ROUND_FILTERS)
            assert p == f.launch_info(capi.INFO_TWO_WAVE_MIN_B) - 1 and p // 64 > f.launch_info(capi.INFO_SIMDS) // 2
        _P.append(p)
    return _P[0]


def skip_mask(B):
    s = np.zeros((F, B), np.uint8)
    s[0, 7::29] = 1
    s[2, 11::13] = 1
    s[F - 1, 12] = 1
    return s


class PoseWindow:
    """F frames of pose rows for B filters on the device; frame(f) = the slices of frame f"""

    def __init__(self, B, prm, nom):
        a, w, dt = imu(B, sum(KC), nom, 32)
        ids = np.zeros((F, B, M), np.int32)
        pos = np.zeros((F, B, M, 3))
        quat = np.zeros((F, B, M, 4))
        for f in range(F):
            ids[f], pos[f], quat[f] = synth.marker_frame(0, B, f, M, nom, prm)
        ids[1, 5] = -1                          # a filter without a marker in one frame
        self.a, self.w, self.dt = to_device(a, F32), to_device(w, F32), to_device(dt, F32)
        self.ids, self.pos, self.quat = to_device(ids, np.int32), to_device(pos, F32), to_device(quat, F32)
        self.skip = to_device(skip_mask(B), np.uint8)
        torch.cuda.synchronize()

    def launch(self, f, mode, record=False):
        return f.frames(KC, self.a, self.w, self.dt, self.ids, self.pos, self.quat, mode, skip=self.skip, record=record)

    def window(self, f, mode, record=False):
        out = self.launch(f, mode, record)
        f.sync()
        return None if not record else [np.ascontiguousarray(np.swapaxes(t.cpu().numpy(), 0, 1)) for t in out]

    def imu_of(self, f):
        k0, K = sum(KC[:f]), KC[f]
        return (self.a[k0:k0 + K], self.w[k0:k0 + K], self.dt[k0:k0 + K]) if K else (None, None, None)

    def fused_frames(self, flt, mode):
        for f in range(F):
            a, w, dt = self.imu_of(f)
            flt.frame(a, w, dt, self.ids[f], self.pos[f], self.quat[f], mode, skip=self.skip[f], fused=True)
        flt.sync()

    def per_call(self, flt, mode):
        for f in range(F):
            a, w, dt = self.imu_of(f)
            if a is not None:
                flt.predict_n(a, w, dt)
            flt.correct(self.ids[f], self.pos[f], self.quat[f], mode, self.skip[f])
        flt.sync()


class MeasWindow:
    """F frames of pixel rows (left / stereo) or corner rows for B filters on the device"""

    def __init__(self, B, nstate, dialect, kind, tilted=False):
        self.kind = kind
        self.prm, nom, rot, P, prev, ids, left, right = perturbed_setup(B, 32, nstate, dialect, kind, tilted=tilted)
        self.state = (nom, rot, P, prev)
        rng = np.random.default_rng(77)
        sd = 2e-4
        a, w, dt = imu(B, sum(KC), nom, 32)
        idsF = np.stack([ids] * F)
        idsF[1, 5] = -1
        idsF[min(2, F - 1), 6, :] = 9           # ids the map does not hold
        leftF = r32(np.stack([left] * F) + rng.normal(0, sd, (F,) + left.shape))
        rightF = r32(np.stack([right] * F) + rng.normal(0, sd, (F,) + right.shape))
        self.a, self.w, self.dt = to_device(a, F32), to_device(w, F32), to_device(dt, F32)
        self.ids, self.left = to_device(idsF, np.int32), to_device(leftF, F32)
        self.right = to_device(rightF, F32) if kind == "stereo" else None
        self.skip = to_device(skip_mask(B), np.uint8)
        self.mk = capi.MEAS_CORNERS if kind == "corners" else capi.MEAS_PIXELS
        self.geo = capi.VIS_CORNERS3D if kind == "corners" else capi.VIS_REFRACTIVE
        torch.cuda.synchronize()

    def launch(self, f, mode=capi.MODE_STACKED, record=False):
        return f.frames_meas(KC, self.a, self.w, self.dt, self.ids, self.left, self.right, self.mk, self.geo, mode, skip=self.skip,
                             record=record)

    def window(self, f, mode=capi.MODE_STACKED, record=False):
        out = self.launch(f, mode, record)
        f.sync()
        return None if not record else [np.ascontiguousarray(np.swapaxes(t.cpu().numpy(), 0, 1)) for t in out]

    def imu_of(self, f):
        k0, K = sum(KC[:f]), KC[f]
        return (self.a[k0:k0 + K], self.w[k0:k0 + K], self.dt[k0:k0 + K]) if K else (None, None, None)

    def fused_frames(self, flt, mode=capi.MODE_STACKED):
        for f in range(F):
            a, w, dt = self.imu_of(f)
            flt.frame_meas(a, w, dt, self.ids[f], self.left[f], None if self.right is None else self.right[f], self.mk, self.geo, mode,
                           skip=self.skip[f])
        flt.sync()

    def per_call(self, flt, mode=capi.MODE_STACKED):
        for f in range(F):
            a, w, dt = self.imu_of(f)
            if a is not None:
                flt.predict_n(a, w, dt)
            r = None if self.right is None else self.right[f]
            if self.kind == "corners":
                flt.correct_corners(self.ids[f], self.left[f], None, self.geo, mode, self.skip[f])
            else:
                flt.correct_pixels(self.ids[f], self.left[f], r, self.skip[f])
        flt.sync()


def tabled(B, prm, nstate, state, policy_batch, dtype=32):
    f = handle(B, prm, dtype, nstate, state, pin=False, policy_batch=policy_batch)
    f.set_noise(rows_of(prm)[np.arange(B) % G])
    return f


def same_handles(x, y):
    return same_state(x.get_state() + (x.applied(),), y.get_state() + (y.applied(),))


# ---- 1. twins -------------------------------------------------------------------------------------------------------------------
POSE = [(0, 18, capi.MODE_NEAREST, 0), (1, 18, capi.MODE_STACKED, 0), (0, 15, capi.MODE_STACKED, 0), (1, 15, capi.MODE_NEAREST, 0),
        (1, 18, capi.MODE_STACKED, 1), (0, 15, capi.MODE_STACKED, 1)]


@pytest.mark.parametrize("record", [False, True])
@pytest.mark.parametrize("dialect,nstate,mode,joseph", POSE)
def test_pose_window_equals_its_twins(dialect, nstate, mode, joseph, record):
    """fails without the resident tabled window: the tabled side then runs the per-call kernels, which differ from the resident twin
    in the last bits"""
    prm, state = state_of(B_ODD, 32, nstate, dialect)
    prm.cov_form = capi.COV_JOSEPH if joseph else capi.COV_SIMPLE
    win = PoseWindow(B_ODD, prm, state[0])
    assert_twin(*run_twins(B_ODD, prm, 32, nstate, state, lambda f: win.window(f, mode, record), pin=False, policy_batch=policy_p()))


MEAS = [("left", capi.MODE_STACKED, 0, 18, False), ("left", capi.MODE_STACKED, 1, 15, True), ("stereo", capi.MODE_STACKED, 1, 18, False),
        ("stereo", capi.MODE_STACKED, 0, 15, False), ("stereo", capi.MODE_STACKED, 0, 18, True), ("corners", capi.MODE_STACKED, 0, 15, False),
        ("corners", capi.MODE_NEAREST, 1, 18, False), ("corners", capi.MODE_STACKED, 1, 18, True), ("corners", capi.MODE_NEAREST, 0, 18, False)]


@pytest.mark.parametrize("record", [False, True])
@pytest.mark.parametrize("kind,mode,dialect,nstate,tilted", MEAS)
def test_meas_window_equals_its_twins(kind, mode, dialect, nstate, tilted, record):
    win = MeasWindow(B_ODD, nstate, dialect, kind, tilted)
    assert_twin(*run_twins(B_ODD, win.prm, 32, nstate, win.state, lambda f: win.window(f, mode, record), pin=False,
                           policy_batch=policy_p()))


# ---- 2. route -------------------------------------------------------------------------------------------------------------------
def test_route_is_reported():
    P = policy_p()
    prm, state = state_of(B_ODD, 32, 18, 0)
    rows = rows_of(prm)[np.arange(B_ODD) % G]
    with BatchedFilter(B_ODD, prm, dtype=32, nstate=18) as f:
        assert f.launch_info(capi.INFO_NOISE_RESIDENT) == 0              # no table
        f.set_policy_batch(P)
        assert f.launch_info(capi.INFO_NOISE_RESIDENT) == 0              # no table, large policy batch
        f.set_noise(rows)
        assert f.launch_info(capi.INFO_NOISE_RESIDENT) == 1
        f.set_team(4, 4)                                                 # ignored while a table is set
        assert f.launch_info(capi.INFO_NOISE_RESIDENT) == 1
        assert f.launch_info(capi.INFO_ROLES_PREDICT, 1) == 1 and f.launch_info(capi.INFO_ROLES_PREDICT, 7) == 1
        assert f.launch_info(capi.INFO_ROLES_MEAS, 4) == 1
        assert f.launch_info(capi.INFO_TEAM_FRAMES) == 0 and f.launch_info(capi.INFO_MEAS_SPLIT, 4) == 0
        f.set_team(0, 0)
        f.loglik_enable(True)
        assert f.launch_info(capi.INFO_NOISE_RESIDENT) == 0              # the sums on: frame by frame
        f.loglik_enable(False)
        assert f.launch_info(capi.INFO_NOISE_RESIDENT) == 1
        f.set_policy_batch(0)
        assert f.launch_info(capi.INFO_NOISE_RESIDENT) == 0              # the handle's own small policy batch
        f.set_policy_batch(f.launch_info(capi.INFO_SIMDS) // 2 * 64)
        assert f.launch_info(capi.INFO_NOISE_RESIDENT) == 0              # exactly half a chip: still the small side
        f.set_policy_batch(f.launch_info(capi.INFO_SIMDS) // 2 * 64 + 1)
        assert f.launch_info(capi.INFO_NOISE_RESIDENT) == 1
        f.set_noise(None)
        assert f.launch_info(capi.INFO_NOISE_RESIDENT) == 0
    with BatchedFilter(B_ODD, prm, dtype=64, nstate=18) as f:
        f.set_policy_batch(P)
        f.set_noise(rows)
        assert f.launch_info(capi.INFO_NOISE_RESIDENT) == 0              # fp64 records


# ---- 3. window == its fused frames --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["pose_stacked", "pose_nearest", "left", "stereo", "corners"])
def test_window_equals_its_fused_frames(what):
    P = policy_p()
    if what.startswith("pose"):
        mode = capi.MODE_STACKED if what == "pose_stacked" else capi.MODE_NEAREST
        prm, state = state_of(B_ODD, 32, 18, 1)
        win = PoseWindow(B_ODD, prm, state[0])
    else:
        mode = capi.MODE_STACKED
        win = MeasWindow(B_ODD, 18, 0, what)
        prm, state = win.prm, win.state
    with tabled(B_ODD, prm, 18, state, P) as a, tabled(B_ODD, prm, 18, state, P) as b:
        assert a.launch_info(capi.INFO_NOISE_RESIDENT) == 1
        win.window(a, mode)
        win.fused_frames(b, mode)
        assert same_handles(a, b)


# ---- 4. identity table at a full round ------------------------------------------------------------------------------------------
def test_identity_table_changes_no_window():
    B, nstate, dialect = 65536, 18, 0
    prm, state = state_of(B, 32, nstate, dialect)
    pose = PoseWindow(B, prm, state[0])
    pix = MeasWindow(B, nstate, dialect, "left")
    with BatchedFilter(B, prm, dtype=32, nstate=nstate) as f0, BatchedFilter(B, prm, dtype=32, nstate=nstate) as f1:
        f1.set_noise(noise.from_params(prm, B))
        assert f1.launch_info(capi.INFO_NOISE_RESIDENT) == 1 and f0.launch_info(capi.INFO_NOISE_RESIDENT) == 0
        for f in (f0, f1):
            f.set_state(*state)
            pose.window(f, capi.MODE_STACKED)
        assert same_handles(f0, f1)
        for f in (f0, f1):
            f.set_state(*state)
            pose.window(f, capi.MODE_NEAREST)
        assert same_handles(f0, f1)
    with BatchedFilter(B, pix.prm, dtype=32, nstate=nstate) as f0, BatchedFilter(B, pix.prm, dtype=32, nstate=nstate) as f1:
        f1.set_noise(noise.from_params(pix.prm, B))
        for f in (f0, f1):
            f.set_state(*pix.state)
            pix.window(f)
        assert same_handles(f0, f1)


# ---- 5. the fall-back routes keep their bits ----------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["pose", "left"])
def test_small_policy_batch_runs_the_per_call_sequence(what):
    if what == "pose":
        prm, state = state_of(B_ODD, 32, 18, 0)
        win = PoseWindow(B_ODD, prm, state[0])
    else:
        win = MeasWindow(B_ODD, 18, 0, what)
        prm, state = win.prm, win.state
    with tabled(B_ODD, prm, 18, state, 0) as a, tabled(B_ODD, prm, 18, state, 0) as b:
        assert a.launch_info(capi.INFO_NOISE_RESIDENT) == 0
        win.window(a, capi.MODE_STACKED)
        win.per_call(b, capi.MODE_STACKED)
        assert same_handles(a, b)


@pytest.mark.parametrize("what", ["pose", "left"])
def test_sums_on_runs_the_per_call_sequence_and_feeds_the_sums(what):
    P = policy_p()
    if what == "pose":
        prm, state = state_of(B_ODD, 32, 18, 0)
        win = PoseWindow(B_ODD, prm, state[0])
    else:
        win = MeasWindow(B_ODD, 18, 0, what)
        prm, state = win.prm, win.state
    with tabled(B_ODD, prm, 18, state, P) as a, tabled(B_ODD, prm, 18, state, P) as b:
        for f in (a, b):
            f.loglik_enable(True)
            f.loglik_reset()
        assert a.launch_info(capi.INFO_NOISE_RESIDENT) == 0
        win.window(a, capi.MODE_STACKED)
        win.per_call(b, capi.MODE_STACKED)
        assert same_handles(a, b)
        la, lb = a.loglik(), b.loglik()
        assert all(np.array_equal(x, y) for x, y in zip(la, lb))
        assert la[2].sum() > 0 and np.all(la[1][la[2] > 0] > 0) and np.all(np.isfinite(la[0]))


def test_joseph_nearest_runs_the_per_call_sequence():
    P = policy_p()
    prm, state = state_of(B_ODD, 32, 18, 1)
    prm.cov_form = capi.COV_JOSEPH
    win = PoseWindow(B_ODD, prm, state[0])
    with tabled(B_ODD, prm, 18, state, P) as a, tabled(B_ODD, prm, 18, state, P) as b:
        assert a.launch_info(capi.INFO_NOISE_RESIDENT) == 1   # the handle-level answer; this call's rows are excluded as without a table
        win.window(a, capi.MODE_NEAREST)
        win.per_call(b, capi.MODE_NEAREST)
        assert same_handles(a, b)


# ---- 6. graph capture -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["pose", "left"])
def test_captured_window_reads_the_rewritten_table(what):
    P = policy_p()
    if what == "pose":
        prm, state = state_of(B_ODD, 32, 18, 0)
        win = PoseWindow(B_ODD, prm, state[0])
    else:
        win = MeasWindow(B_ODD, 18, 0, what)
        prm, state = win.prm, win.state
    rows = rows_of(prm)
    t1, t2 = rows[np.arange(B_ODD) % G], rows[(np.arange(B_ODD) + 2) % G]
    with handle(B_ODD, prm, 32, 18, state, pin=False, policy_batch=P) as gph:
        gph.set_noise(t1)
        assert gph.launch_info(capi.INFO_NOISE_RESIDENT) == 1
        gid = gph.graph_capture(lambda: win.launch(gph, capi.MODE_STACKED))
        for t in (t1, t2):
            gph.set_state(*state)
            gph.set_noise(t)                    # rewritten in place: the graph reads the values current at its replay
            gph.graph_launch(gid)
            gph.sync()
            with handle(B_ODD, prm, 32, 18, state, pin=False, policy_batch=P) as ref:
                ref.set_noise(t)
                win.window(ref, capi.MODE_STACKED)
                assert same_handles(gph, ref)
    # the two tables give different results (a graph that kept the first table's values would fail above)
    with tabled(B_ODD, prm, 18, state, P) as x:
        win.window(x, capi.MODE_STACKED)
        with handle(B_ODD, prm, 32, 18, state, pin=False, policy_batch=P) as y:
            y.set_noise(t2)
            win.window(y, capi.MODE_STACKED)
            assert not np.array_equal(x.get_state()[0], y.get_state()[0])


# ---- 7. the sweep on the recording ----------------------------------------------------------------------------------------------
def test_sweep_on_the_recording_equals_its_twins():
    P = policy_p()
    d = np.load(os.path.join(GOLD, "recordings.npz"))
    imu_, image = d["land_imu"], d["land_image"]
    t = image[:, 0]
    keep = ~(((t > t[0] + 8.0) & (t < t[0] + 8.4)) | ((t > t[0] + 20.0) & (t < t[0] + 20.25)))
    image = image[keep]
    prm = capi.default_params(0)
    rows = rows_of(prm)
    B = 320
    g = np.arange(B) % G
    with BatchedFilter(B, prm, dtype=32) as flt:
        flt.set_policy_batch(P)
        flt.set_noise(rows[g])
        assert flt.launch_info(capi.INFO_NOISE_RESIDENT) == 1
        replay.replay_windowed(flt, imu_, image, prm)
        got = flt.get_state()
        got_app = flt.applied()
    ends = []
    for k in range(G):
        with BatchedFilter(B, with_row(prm, rows[k]), dtype=32) as twin:
            twin.set_policy_batch(P)
            replay.replay_windowed(twin, imu_, image, with_row(prm, rows[k]))
            ref = twin.get_state()
            ref_app = twin.applied()
        sel = g == k
        assert same_state([x[sel] for x in got], [x[sel] for x in ref]), f"row {k}"
        assert np.array_equal(got_app[sel], ref_app[sel])
        ends.append(ref[0][0].astype(np.float64))
    spread = min(state_rel_err_literal(ends[i][None], ends[j][None]) for i in range(G) for j in range(G) if i != j)
    print(f"sweep fp32, resident tabled windows: smallest row-to-row difference of the end states {spread:.2e}")
    assert spread > 1e-3                        # an ignored table cannot pass: the rows' twins end far apart
