"""The cells of the route walks: handle states, the documented route rules restated, call shapes, shared inputs and the calls through the
frame and window entry points, at a small batch placed in each size class with set_policy_batch.  Used by tests/test_routes_gpu.py (which
asserts on about a hundred cells at B = 128), by tests/test_independence_gpu.py (the same cells at B = 193, each filter moved, cut off, left
alone or set beside broken neighbours) and by tools/route_matrix.py (which prints every cell for comparing two builds).  The scenes come from
the suite's own builders."""
import numpy as np
import torch

from fbus_ekf import BatchedFilter, capi, synth
from support import G, env, imu, perturbed_setup, poisoned_state, r32, rows_of, state_of, to_device, update_call, with_nan

B = 128
KC = (3, 0, 2)                          # IMU samples in front of each frame: unequal, one frame without any
NEAREST, STACKED = capi.MODE_NEAREST, capi.MODE_STACKED
KINDS = (capi.KERNEL_PREDICT, capi.KERNEL_CORRECT, capi.KERNEL_PREDICT_N, capi.KERNEL_MARKER_POSE, capi.KERNEL_FRAME, capi.KERNEL_CORRECT_CORNERS)


# ---- handle states ----------------------------------------------------------------------------------------------------------------------
# size class: the policy batch in tiles against the device's SIMDs -- Q: a quarter, H: exactly half, H1: half + 1, R: one round, R+1: one more;
# or the policy batch itself
def policy_batch(f, size):
    if isinstance(size, int):                            # (a number of filters as it is)
        return size
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


# ---- the documented rules, restated from the handle's own launch_info answers -----------------------------------------------------------------
def frame_route(f, cfg, kind, mode, M, K):
    fp32, tabled = cfg.dtype == 32, cfg.noise or cfg.lik
    if tabled and not (f.launch_info(capi.INFO_NOISE_RESIDENT) and K <= 255):
        return "per_call"
    if kind == "pose":
        if cfg.joseph and mode == NEAREST:
            return "per_call"
        if not fp32:
            return "f64_fused" if mode == STACKED and not cfg.joseph and 1 <= K <= 255 else "per_call"
        if tabled:
            return "tabled_resident"
        return "team" if f.launch_info(capi.INFO_TEAM_FRAMES) and K <= 255 else "fused"
    if not fp32 or M == 0 or K > 255 or cfg.env.get("FBUS_NO_FRAME_MEAS") == "1":
        return "per_call"
    if tabled:
        return "tabled_resident"
    roles = 1 if (kind == "corners" and mode == NEAREST) else f.launch_info(capi.INFO_ROLES_MEAS, M)
    return "meas_resident" if roles == 1 else "per_call"


def window_route(f, cfg, kind, mode, M, nframes, rows):
    r = frame_route(f, cfg, kind, mode, M, 1)
    if r in ("per_call", "f64_fused") or (kind != "pose" and nframes == 1):
        return "by_frame"
    if r == "team":
        return "team_frames" if rows else "team"
    return "one_wave"


# ---- call shapes ---------------------------------------------------------------------------------------------------------------------------------
# (kind, mode, M, kcount, rows): every kind with and without rows, a one-frame window, M = 0 and M = 1
WINDOWS = [("pose", STACKED, 4, KC, False), ("pose", STACKED, 4, KC, True), ("pose", NEAREST, 4, KC, True), ("pose", STACKED, 0, KC, False),
           ("left", STACKED, 4, KC, False), ("stereo", STACKED, 4, KC, True), ("corners", NEAREST, 4, KC, False),
           ("corners", STACKED, 4, KC, True), ("left", STACKED, 1, KC, True), ("stereo", STACKED, 0, KC, False),
           ("stereo", STACKED, 4, (2,), True)]


def shapes_of(cfg):
    """a third of the shapes per handle state, every shape on the states that differ most (about a hundred cells in all)"""
    i = CFGS.index(cfg)
    return WINDOWS if i in (0, 1, 7, 12) else list(dict.fromkeys(WINDOWS[i % 3::3] + WINDOWS[:2]))


# ---- inputs: computed once per (record type, state size, dialect), shared, never written -----------------------------------------------------
_DATA = {}


class Data:
    """three frames of pose rows and of pixel / corner rows for B filters, 300 IMU samples with one shared period (dt) and with a period
    per filter (dt_b).  Everything per filter belongs to the filter's IDENTITY (self.ids; 0 .. B here): take() and the other derivations
    below carry it along, so the same filter sees the same inputs wherever it stands.  The numpy half (self.h, self.state,
    self.meas_state) needs no GPU; device=True uploads it (self.a, self.w, self.dt, self.dt_b, self.skip, self.rows)."""

    def __init__(self, dtype, nstate, dialect, B=B, device=True):
        self.B, self.dtype, self.ids = B, dtype, np.arange(B)
        F = len(KC)
        self.prm, state = state_of(B, dtype, nstate, dialect)
        nom = state[0]
        a, w, dt = imu(B, 300, nom, dtype)
        dt_b = r32(np.random.default_rng(78).uniform(0.003, 0.007, (300, B)))
        ids = np.zeros((F, B, 4), np.int32)
        pos, quat = np.zeros((F, B, 4, 3)), np.zeros((F, B, 4, 4))
        for f in range(F):
            ids[f], pos[f], quat[f] = synth.marker_frame(0, B, f, 4, nom, self.prm)
        ids[1, 5] = -1                                   # a filter without a marker in one frame
        skip = np.zeros((F, B), np.uint8)
        skip[0, self.ids % 29 == 7] = 1
        skip[F - 1, self.ids == 12] = 1
        rows = {"pose": (ids, pos, quat)}
        rng = np.random.default_rng(77)
        for kind in ("stereo", "corners"):
            prm, mnom, rot, P, prev, mids, left, right = perturbed_setup(B, dtype, nstate, dialect, kind, n=B)
            idsF = np.stack([mids] * F)
            idsF[1, 5] = -1
            noisy = lambda x: np.stack([x] * F) + rng.normal(0, 2e-4, (F,) + x.shape)
            rows[kind] = (idsF, noisy(left), noisy(right) if kind == "stereo" else None)
            self.meas_prm, meas_state = prm, (mnom, rot, P, prev)
        self.h = {"state": state, "meas_state": meas_state, "a": a, "w": w, "dt": dt, "dt_b": dt_b, "skip": skip, "rows": rows}
        self._finish(device)

    def _finish(self, device, view=None):
        """the device half: uploaded, or (view = (owner, lo, hi)) filters lo .. hi of the owner's tensors"""
        self.state, self.meas_state = self.h["state"], self.h["meas_state"]
        self.src, self.lo, self.hi = view or (self if device else None, 0, self.B)
        if device and view is None:
            npd, h = np.float32 if self.dtype == 32 else np.float64, self.h
            self.a, self.w, self.dt, self.dt_b = (to_device(h[k], npd) for k in ("a", "w", "dt", "dt_b"))
            self.skip = to_device(h["skip"], np.uint8)
            self.rows = {k: (to_device(i, np.int32), to_device(x, npd), to_device(y, npd)) for k, (i, x, y) in h["rows"].items()}
            self.rows["left"] = self.rows["stereo"][:2] + (None,)
            torch.cuda.synchronize()

    def _derived(self, h, ids, view=None):
        d = object.__new__(Data)
        d.B, d.dtype, d.ids, d.prm, d.meas_prm, d.h = len(ids), self.dtype, ids, self.prm, self.meas_prm, h
        d._finish(self.src is not None, view)
        return d

    def _each(self, fn):
        """the numpy half with fn(array, its filter axis) in place of every per-filter array"""
        h = self.h
        return {"state": tuple(fn(x, 0) for x in h["state"]), "meas_state": tuple(fn(x, 0) for x in h["meas_state"]),
                "a": fn(h["a"], 1), "w": fn(h["w"], 1), "dt": h["dt"], "dt_b": fn(h["dt_b"], 1), "skip": fn(h["skip"], 1),
                "rows": {k: tuple(None if x is None else fn(x, 1) for x in v) for k, v in h["rows"].items()}}

    def take(self, filter_ids):
        """the same scene for the filters at `filter_ids` of this one, in that order.  A run lo .. hi is served from this scene's own device
        tensors (one_frame passes slices of them, window gathers); any other order is uploaded afresh"""
        pos = np.asarray(filter_ids, np.int64)
        run = self.src is not None and np.array_equal(pos, np.arange(pos[0], pos[0] + len(pos)))
        view = (self.src, self.lo + int(pos[0]), self.lo + int(pos[0]) + len(pos)) if run else None
        return self._derived(self._each(lambda x, ax: np.take(x, pos, axis=ax)), self.ids[pos], view)

    def poisoned(self, S, form):
        """the filters at S broken, S[i] in the way form[i] (support.poisoned_state: a b c e; d: finite state, NaN measurement rows, IMU
        samples and dt_b entries); ids, skip and the shared dt as they are"""
        S, form = np.asarray(S), np.asarray(form)
        h = self._each(lambda x, ax: x)
        for key in ("state", "meas_state"):
            h[key] = poisoned_state(*h[key][:3], S, form) + h[key][3:]
        nan = lambda x: None if x is None else with_nan(x, S[form == 3], 1)
        h["a"], h["w"], h["dt_b"] = nan(h["a"]), nan(h["w"]), nan(h["dt_b"])
        h["rows"] = {k: (i, nan(x), nan(y)) for k, (i, x, y) in h["rows"].items()}
        return self._derived(h, self.ids)

    def absent(self, where, how):
        """the filters at `where` without a measurement in any frame: how = "skip": their skip bytes set, "ids": all their ids -1"""
        h = self._each(lambda x, ax: x)
        if how == "skip":
            h["skip"] = h["skip"].copy()
            h["skip"][:, where] = 1
        else:
            h["rows"] = {k: (i.copy(), x, y) for k, (i, x, y) in h["rows"].items()}
            for i, _, _ in h["rows"].values():
                i[:, where] = -1
        return self._derived(h, self.ids)

    def with_outliers(self):
        """slot 0 of every frame 30 sigma off on the filters id % 8 == 5: one corner of it in every coordinate (a corner on a reflection; a
        rigid shift of all four would be taken up by the prior's pose uncertainty), the position of a pose row"""
        bad = self.ids % 8 == 5
        h = self._each(lambda x, ax: x)
        h["rows"] = {k: (i, x.copy(), y) for k, (i, x, y) in h["rows"].items()}
        for kind, (_, x, _) in h["rows"].items():
            n, sigma = (2, self.meas_prm.r_pix) if kind == "stereo" else (3, self.meas_prm.r_pos if kind == "corners" else self.prm.r_pos)
            x[:, bad, 0, 0:n] += 30 * np.sqrt(sigma)
        return self._derived(h, self.ids)


def data_of(cfg, B=B):
    key = (cfg.dtype, cfg.nstate, cfg.dialect, B)
    if key not in _DATA:
        _DATA[key] = Data(*key)
    return _DATA[key]


def make(cfg, d, meas, filters=None):
    """a handle in the cell's state, timing on, for the filters `filters` of the job (their number: the batch; their ids: the noise rows):
    by default 0 .. d.B"""
    filters = np.arange(d.B) if filters is None else np.asarray(filters)
    B = len(filters)
    prm = capi.FbusParams.from_buffer_copy(d.meas_prm if meas else d.prm)
    prm.cov_form = capi.COV_JOSEPH if cfg.joseph else capi.COV_SIMPLE
    with env(**cfg.env):                                  # (read once, at create)
        f = BatchedFilter(B, prm, device=0, dtype=cfg.dtype, nstate=cfg.nstate)
    f.set_state(*(d.meas_state if meas else d.state))
    f.set_team(*cfg.team)
    f.set_policy_batch(policy_batch(f, cfg.size))
    if cfg.noise:
        f.set_noise(rows_of(prm)[filters % G])
    if cfg.lik:
        f.loglik_enable(True)
    f.timing_enable(True)
    return f


# ---- calls -----------------------------------------------------------------------------------------------------------------------------------
def frame_rows(d, kind, fr, M):
    """(ids, a, b, skip) of frame fr for d's filters: SLICES of the arrays a handle of all the owner's filters would be given"""
    lo, hi = d.lo, d.hi
    cut = lambda x: None if x is None else x[fr, :, :M].contiguous()[lo:hi]
    ids, a, b = (cut(x) for x in d.src.rows[kind])
    return ids, a, b, d.src.skip[fr, lo:hi]


def imu_of(d, k0, k1, per):
    """samples k0 .. k1 for d's filters with the shared period, or per: each filter's own"""
    s, lo, hi = d.src, d.lo, d.hi
    return (s.a[k0:k1, lo:hi].contiguous(), s.w[k0:k1, lo:hi].contiguous(),
            s.dt_b[k0:k1, lo:hi].contiguous() if per else s.dt[k0:k1])


def one_frame(f, d, kind, mode, M, K, fr=0, k0=0, per=False):
    ids, a, b, skip = frame_rows(d, kind, fr, M)
    acc, gyr, dt = imu_of(d, k0, k0 + K, per) if K else (None, None, None)
    if M == 0:
        ids = a = b = None
    if kind == "pose":
        f.frame(acc, gyr, dt, ids, a, b, mode, skip=skip, fused=True)
    else:
        mk, geo = (capi.MEAS_CORNERS, capi.VIS_CORNERS3D) if kind == "corners" else (capi.MEAS_PIXELS, capi.VIS_REFRACTIVE)
        f.frame_meas(acc, gyr, dt, ids, a, b, mk, geo, mode, skip=skip)


def window(f, d, kind, mode, M, kc, rows, per=False):
    F, Kt = len(kc), sum(kc)
    s, lo, hi = d.src, d.lo, d.hi
    ids, a, b = (None if x is None else x[:F, lo:hi, :M].contiguous() for x in s.rows[kind])
    if M == 0:
        ids = a = b = None
    acc, gyr, dt = imu_of(d, 0, Kt, per)
    skip = s.skip[:F, lo:hi].contiguous()
    if kind == "pose":
        return f.frames(kc, acc, gyr, dt, ids, a, b, mode, skip=skip, record=rows)
    mk, geo = (capi.MEAS_CORNERS, capi.VIS_CORNERS3D) if kind == "corners" else (capi.MEAS_PIXELS, capi.VIS_REFRACTIVE)
    return f.frames_meas(kc, acc, gyr, dt, ids, a, b, mk, geo, mode, skip=skip, record=rows)


def update_nis(f, d, kind, mode, M, fr=0):
    """the per-call update of frame fr through its NIS entry point: (nis, dof)"""
    ids, a, b, skip = frame_rows(d, kind, fr, M)
    return update_call(f, kind, ids, a, b, nis=True, mode=mode, skip=skip)
