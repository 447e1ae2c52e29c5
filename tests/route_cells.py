"""The cells of the route walks: handle states, shared inputs and the calls through the frame and window entry points, at a small batch
placed in each size class with set_policy_batch.  Used by tests/test_routes_gpu.py (which asserts on about a hundred cells) and by
tools/route_matrix.py (which prints every cell for comparing two builds).  The scenes come from the suite's own builders."""
import numpy as np
import torch

from fbus_ekf import BatchedFilter, capi, synth
from support import G, env, imu, perturbed_setup, rows_of, state_of, to_device

B = 128
KC = (3, 0, 2)                          # IMU samples in front of each frame: unequal, one frame without any
NEAREST, STACKED = capi.MODE_NEAREST, capi.MODE_STACKED
KINDS = (capi.KERNEL_PREDICT, capi.KERNEL_CORRECT, capi.KERNEL_PREDICT_N, capi.KERNEL_MARKER_POSE, capi.KERNEL_FRAME, capi.KERNEL_CORRECT_CORNERS)


# ---- handle states ----------------------------------------------------------------------------------------------------------------------
# size class: the policy batch in tiles against the device's SIMDs -- Q: a quarter, H: exactly half, H1: half + 1, R: one round, R+1: one more
def policy_batch(f, size):
    simds = f.launch_info(capi.INFO_SIMDS)
    return 64 * {"Q": simds // 4, "H": simds // 2, "H1": simds // 2 + 1, "R": simds, "R+1": simds + 1}[size]


class Cfg:
    def __init__(self, name, size, dtype=32, nstate=18, dialect=0, joseph=False, noise=False, lik=False, team=(0, 0), env=None):
        self.name, self.size, self.dtype, self.nstate, self.dialect, self.joseph = name, size, dtype, nstate, dialect, joseph
        self.noise, self.lik, self.team, self.env = noise, lik, team, env or {}

    def __repr__(self):
        return self.name


CFGS = [
    Cfg("f32 half", "H"), Cfg("f32 half+1", "H1"), Cfg("f32 n15 cpp quarter", "Q", nstate=15, dialect=1),
    Cfg("f32 set_team(1,1) quarter", "Q", team=(1, 1)), Cfg("f32 set_team(4,4) round", "R", team=(4, 4)),
    Cfg("f32 joseph half+1", "H1", joseph=True), Cfg("f32 joseph half", "H", joseph=True),
    Cfg("f32 noise half+1", "H1", noise=True), Cfg("f32 noise half", "H", noise=True), Cfg("f32 noise n15 round", "R", nstate=15, noise=True),
    Cfg("f32 noise lik round", "R", noise=True, lik=True), Cfg("f32 lik half+1", "H1", lik=True),
    Cfg("f64 half+1", "H1", dtype=64), Cfg("f64 joseph half+1", "H1", dtype=64, joseph=True), Cfg("f64 noise round", "R", dtype=64, noise=True),
    Cfg("f32 TEAM_FRAME=2 set_team(1,1) round", "R", team=(1, 1), env={"FBUS_TEAM_FRAME": "2"}),
    Cfg("f32 TEAM_FRAME=1 quarter", "Q", env={"FBUS_TEAM_FRAME": "1"}),
    Cfg("f32 NO_FRAME_MEAS round", "R", env={"FBUS_NO_FRAME_MEAS": "1"}),
    Cfg("f32 MEAS_SPLIT=0 quarter", "Q", env={"FBUS_MEAS_SPLIT": "0"}),
]


# ---- inputs: computed once per (record type, state size, dialect), shared, never written -----------------------------------------------------
_DATA = {}


class Data:
    """three frames of pose rows and of pixel / corner rows for B filters on the device, and 300 IMU samples"""

    def __init__(self, dtype, nstate, dialect, B=B):
        self.B = B
        npd = np.float32 if dtype == 32 else np.float64
        F = len(KC)
        self.prm, self.state = state_of(B, dtype, nstate, dialect)
        nom = self.state[0]
        a, w, dt = imu(B, 300, nom, dtype)
        self.a, self.w, self.dt = to_device(a, npd), to_device(w, npd), to_device(dt, npd)
        ids = np.zeros((F, B, 4), np.int32)
        pos, quat = np.zeros((F, B, 4, 3)), np.zeros((F, B, 4, 4))
        for f in range(F):
            ids[f], pos[f], quat[f] = synth.marker_frame(0, B, f, 4, nom, self.prm)
        ids[1, 5] = -1                                   # a filter without a marker in one frame
        skip = np.zeros((F, B), np.uint8)
        skip[0, 7::29] = 1
        skip[F - 1, 12] = 1
        self.skip = to_device(skip, np.uint8)
        self.rows = {"pose": (to_device(ids, np.int32), to_device(pos, npd), to_device(quat, npd))}
        rng = np.random.default_rng(77)
        for kind in ("stereo", "corners"):
            prm, mnom, rot, P, prev, mids, left, right = perturbed_setup(B, dtype, nstate, dialect, kind, n=B)
            idsF = np.stack([mids] * F)
            idsF[1, 5] = -1
            noisy = lambda x: np.stack([x] * F) + rng.normal(0, 2e-4, (F,) + x.shape)
            self.rows[kind] = (to_device(idsF, np.int32), to_device(noisy(left), npd), to_device(noisy(right), npd) if kind == "stereo" else None)
            self.meas_prm, self.meas_state = prm, (mnom, rot, P, prev)
        self.rows["left"] = self.rows["stereo"][:2] + (None,)
        torch.cuda.synchronize()


def data_of(cfg):
    key = (cfg.dtype, cfg.nstate, cfg.dialect)
    if key not in _DATA:
        _DATA[key] = Data(*key)
    return _DATA[key]


def make(cfg, d, meas):
    """a handle in the cell's state, timing on"""
    B = d.B
    prm = capi.FbusParams.from_buffer_copy(d.meas_prm if meas else d.prm)
    prm.cov_form = capi.COV_JOSEPH if cfg.joseph else capi.COV_SIMPLE
    with env(**cfg.env):                                  # (read once, at create)
        f = BatchedFilter(B, prm, device=0, dtype=cfg.dtype, nstate=cfg.nstate)
    f.set_state(*(d.meas_state if meas else d.state))
    f.set_team(*cfg.team)
    f.set_policy_batch(policy_batch(f, cfg.size))
    if cfg.noise:
        f.set_noise(rows_of(prm)[np.arange(B) % G])
    if cfg.lik:
        f.loglik_enable(True)
    f.timing_enable(True)
    return f


# ---- calls -----------------------------------------------------------------------------------------------------------------------------------
def one_frame(f, d, kind, mode, M, K, fr=0, k0=0):
    ids, a, b = d.rows[kind]
    ids, a, b = ids[fr, :, :M].contiguous(), a[fr, :, :M].contiguous(), None if b is None else b[fr, :, :M].contiguous()
    acc, gyr, dt = (d.a[k0:k0 + K], d.w[k0:k0 + K], d.dt[k0:k0 + K]) if K else (None, None, None)
    if M == 0:
        ids = a = b = None
    if kind == "pose":
        f.frame(acc, gyr, dt, ids, a, b, mode, skip=d.skip[fr], fused=True)
    else:
        mk, geo = (capi.MEAS_CORNERS, capi.VIS_CORNERS3D) if kind == "corners" else (capi.MEAS_PIXELS, capi.VIS_REFRACTIVE)
        f.frame_meas(acc, gyr, dt, ids, a, b, mk, geo, mode, skip=d.skip[fr])


def window(f, d, kind, mode, M, kc, rows):
    F, Kt = len(kc), sum(kc)
    ids, a, b = d.rows[kind]
    ids, a, b = ids[:F, :, :M].contiguous(), a[:F, :, :M].contiguous(), None if b is None else b[:F, :, :M].contiguous()
    if M == 0:
        ids = a = b = None
    acc, gyr, dt = d.a[:Kt], d.w[:Kt], d.dt[:Kt]
    if kind == "pose":
        return f.frames(kc, acc, gyr, dt, ids, a, b, mode, skip=d.skip[:F].contiguous(), record=rows)
    mk, geo = (capi.MEAS_CORNERS, capi.VIS_CORNERS3D) if kind == "corners" else (capi.MEAS_PIXELS, capi.VIS_REFRACTIVE)
    return f.frames_meas(kc, acc, gyr, dt, ids, a, b, mk, geo, mode, skip=d.skip[:F].contiguous(), record=rows)
