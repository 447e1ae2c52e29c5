"""GPU suite: IMU samples at the edges of predict_nominal's domain (fbus-ekf_amd/csrc/ekf_device.hpp) through every route that predicts.

The scene is tests/imu_edges.py: B = 193 filters, K = 7 samples, sixteen classes of (rate, period) -- zero and denormal-square rates, both
sides of the C++ dialect's small-rate guard, both sides of the 0.5 rad switch between the sin/cos polynomials and the library, gaps of a
second, zero and negative periods -- interleaved so that every wave holds every class at every sample and every filter changes branch from
sample to sample; once with a period per filter and once with a shared period.  The expected values are the C oracle's (fbo_predict),
held to util.assert_parity's own gates: the standard ones for fp32 records, dtype = 64 for fp64 records.  tests/test_imu_edges_cpu.py
shows that fp32 records lose a tenth of those gates at most on this scene and that the gates refuse six wrong variants of the step.

Every handle state of STATES (its own list: tests/route_cells.py's CFGS is what the route and independence suites time and count) runs
  1 predict     sample by sample, the state against the oracle after EVERY sample; where a sample's rate is zero or its square below the
                smallest normal fp32 number: the quaternion moved by less than 1e-6 and the records are finite
  2 predict_n   K = 7 in one call, against the oracle and against cell 1 (the figures of test_predict_n_equals_repeated_predict, which
                holds the two to fp32 rounding, nowhere to the bit)
  3 frame       a pose frame with M = 0 through the fused entry point
  4 windows     kcount = (3, 0, 4) with M = 0, with and without trajectory rows: the rows against the oracle's state after each frame, the
                window against its frames bit for bit (team windows against team frames, one-wave against one-wave)
  5 meas        frame_meas and frames_meas with M = 1 and every id -1 for left pixels, stereo pixels and corners: the predicted record,
                applied == 0
  6 graph       one captured replay of a fused frame equals the eager run bit for bit (one handle state)
and, fp64 records only, ONE sample of imu_edges.guard_probe (9e-5 rad/s over 64 s: the only input on which the fp64 gate tells the guard
of the small-rate branch from one a decade lower).

predict_nominal's call sites and the cells that run them (the route names are asserted; the launch counts of timing_read and the roles of
launch_info say which kernel family ran):
  ekf_kernels.hpp:632   predict_kernel, K = 1         cell 1 where launch_info(INFO_ROLES_PREDICT, 1) == 1: half+1, round+1, set_team(1,1),
                                                      TEAM_FRAME=2 set_team(1,1), noise, fp64 (the scalar fp64 form)
  ekf_team.hpp:199      predict_team_kernel           cell 1 elsewhere: quarter, 193 filters, set_team(4,4), TEAM_FRAME=1 quarter
  ekf_kernels.hpp:409   predict_steps in predict_kernel (K > 1: cell 2 where launch_info(INFO_ROLES_PREDICT, 7) == 1; the parked form at
                        round+1 and for fp64), frame_kernel (cell 3 "fused" below round+1), frames_kernel (cell 4 "one_wave"; with the
                        noise table: cells 3 - 5 "tabled_resident")
  ekf_kernels.hpp:1167  frame2_kernel                 cell 3 "fused" at round+1 (FBUS_X_PACK_2W), "f64_fused" (fp64)
  ekf_team.hpp:374      predict_n_team_kernel         cell 2 where the roles are 4; cell 5 where its route is "per_call"
  ekf_team.hpp:868      frames_team_kernel            cells 3 and 4 "team" / "team_frames": quarter, 193 filters, set_team(4,4), TEAM_FRAME=2
  ekf_meas.hpp:1976     frame_meas_kernel             cell 5 "meas_resident": packed for left pixels and corners and for the Matlab
                                                      dialect's stereo pixels, the scalar form for the C++ dialect's stereo pixels
The last test shows that the cells reach every value of both route enums and every family above."""
import copy

import numpy as np
import pytest
import torch

import imu_edges as ie
from fbus_ekf import capi, noise
from route_cells import KINDS, NEAREST, STACKED, Cfg, frame_route, imu_of, make, one_frame, policy_batch, window, window_route
from support import same_state, to_device
from util import assert_parity, cov_rel_err, cov_rel_err_blockwise, state_rel_err

pytestmark = pytest.mark.gpu

B, K = ie.B, ie.K
KC = (3, 0, 4)                                # the K samples as three frames: unequal, one frame without any
MEAS = ("left", "stereo", "corners")


# ---- handle states: (name, size class, the fused frame's route, roles of predict and of predict_n) --------------------------------------------
def _state(name, size, frame, roles, n=18, dialect=0, **kw):
    cfg = Cfg(f"{name}{' n15' if n == 15 else ''}{' cpp' if dialect else ''}", size, nstate=n, dialect=dialect, **kw)
    cfg.frame, cfg.roles = frame, roles
    return cfg


def _states(name, size, frame, roles, variants, **kw):
    return [_state(name, size, frame, roles, n, d, **kw) for n, d in variants]


STATES = (_states("f32 quarter", "Q", "team", (3, 4), [(18, 0), (18, 1), (15, 0), (15, 1)])
          + _states("f32 half+1", "H1", "fused", (1, 1), [(18, 0), (18, 1), (15, 1)])
          + _states("f32 round+1", "R+1", "fused", (1, 1), [(18, 0), (18, 1), (15, 0)])
          + _states("f32 set_team(1,1) quarter", "Q", "fused", (1, 1), [(18, 0), (15, 1)], team=(1, 1))
          + _states("f32 set_team(4,4) round", "R", "team", (4, 4), [(18, 0), (18, 1)], team=(4, 4))
          + _states("f32 193 filters", B, "team", (3, 4), [(18, 0), (15, 1)])
          + _states("f64 half+1", "H1", "f64_fused", (1, 1), [(18, 0), (18, 1), (15, 1)], dtype=64)
          + _states("f32 TEAM_FRAME=1 quarter", "Q", "fused", (3, 4), [(18, 0), (18, 1)], env={"FBUS_TEAM_FRAME": "1"})
          + _states("f32 TEAM_FRAME=2 set_team(1,1) round", "R", "team", (1, 1), [(18, 1), (15, 0)], team=(1, 1), env={"FBUS_TEAM_FRAME": "2"})
          + _states("f32 noise half+1", "H1", "tabled_resident", (1, 1), [(18, 0), (18, 1)], noise=True)
          + _states("f32 noise round", "R", "tabled_resident", (1, 1), [(15, 0)], noise=True))
WINDOW_OF = {"team": ("team", "team_frames"), "fused": ("one_wave", "one_wave"), "tabled_resident": ("one_wave", "one_wave"),
             "f64_fused": ("by_frame", "by_frame"), "per_call": ("by_frame", "by_frame")}     # (without rows, with rows)


# ---- the scene on the device, shaped like route_cells.Data -----------------------------------------------------------------------------------
class EdgeData:
    """what route_cells.make, one_frame and window read of a Data: the scene's initial state as pose state and as measurement state, its
    IMU samples with the shared period (dt) and the per-filter one (dt_b), and three frames of M = 1 rows whose ids are all -1"""

    def __init__(self, dtype, nstate, dialect, guard=False):
        s = self.scene = (ie.guard_probe if guard else ie.scene)(nstate, dialect)
        self.B, self.dtype, self.ids = B, dtype, np.arange(B)
        self.prm = self.meas_prm = s.prm
        self.state = self.meas_state = s.state
        npd, F = (np.float32 if dtype == 32 else np.float64), len(KC)
        self.a, self.w, self.dt, self.dt_b = (to_device(np.array(x), npd) for x in (s.acc, s.gyr, s.dt["shared"], s.dt["per"]))   # (copies: the scene is read-only)
        self.skip = to_device(np.zeros((F, B), np.uint8))
        none = to_device(np.full((F, B, 1), -1, np.int32))
        zeros = lambda w: to_device(np.zeros((F, B, 1, w), npd))
        self.rows = {"pose": (none, zeros(3), zeros(4)), "stereo": (none, zeros(8), zeros(8)), "corners": (none, zeros(12), None)}
        self.rows["left"] = self.rows["stereo"][:2] + (None,)
        self.src, self.lo, self.hi = self, 0, B
        torch.cuda.synchronize()


_DATA = {}


def data_of(cfg, guard=False):
    key = (cfg.dtype, cfg.nstate, cfg.dialect, guard)
    if key not in _DATA:
        _DATA[key] = EdgeData(*key)
    return _DATA[key]


def handle(cfg, d, meas=False):
    """route_cells.make; a tabled state gets a table whose rows all equal the handle's parameters, so the oracle needs none"""
    plain = copy.copy(cfg)
    plain.noise = False
    f = make(plain, d, meas)
    if cfg.noise:
        f.set_noise(np.tile(noise.row_of(d.prm), (B, 1)))
    return f


def counts(f):
    return {k: f.timing_read(k)[1] for k in KINDS}


def launches(**kw):
    """{kernel kind: launches} with the named kinds (predict, predict_n, frame, update) set and every other zero"""
    names = {"predict": capi.KERNEL_PREDICT, "predict_n": capi.KERNEL_PREDICT_N, "frame": capi.KERNEL_FRAME,
             "update": capi.KERNEL_CORRECT_CORNERS}
    n = dict.fromkeys(KINDS, 0)
    n.update({names[k]: v for k, v in kw.items()})
    return n


# ---- expectations ------------------------------------------------------------------------------------------------------------------------
class Cells:
    """the cells of one handle state: every one is run, the failures are printed with the classes that carry them and counted"""

    def __init__(self, cfg):
        self.cfg, self.d, self.failed, self.n = cfg, data_of(cfg), [], 0

    def run(self, what, fn):
        self.n += 1
        try:
            fn()
        except AssertionError as e:
            print(f"FAILED {self.cfg}: {what}: {str(e).splitlines()[0] if str(e) else ''}")
            self.failed.append(what)

    def against_oracle(self, got, stream, samples, what, guard=False):
        """util.assert_parity against the oracle's state after `samples` samples; on a failure the figures class by class"""
        cfg = self.cfg
        ref = ie.reference(cfg.nstate, cfg.dialect, stream, guard)[samples]
        assert all(np.isfinite(x).all() for x in got[:3]), f"{what}: not finite"
        try:
            return assert_parity(got, ref, cfg.dtype, f"{cfg}: {what}", verbose=False)
        except AssertionError:
            if not guard:
                ie.print_classes(what, got, ref, self.d.scene, samples, ie.GATES if cfg.dtype == 32 else ie.GATES_F64)
            raise

    def done(self):
        assert not self.failed, f"{len(self.failed)} of {self.n} cells: {self.failed}"


def per_call(cells, stream, worst):
    """cell 1 -> the state after the K samples"""
    cfg, d, s, per = cells.cfg, cells.d, cells.d.scene, stream == "per"
    with handle(cfg, d) as f:
        before = f.get_state()
        for k in range(K):
            f.predict(*imu_of(d, k, k + 1, per))
            got = f.get_state()
            e = cells.against_oracle(got, stream, k + 1, f"predict, {stream}, sample {k}")
            for name in ie.GATES:
                worst[name] = max(worst.get(name, 0.0), e[name])
            still = s.w2[k] < ie.DENORMAL                              # zero and denormal-square rates: the identity, not NaN
            assert np.abs(got[0][still, 6:10].astype(np.float64) - before[0][still, 6:10]).max() < 1e-6, f"sample {k}: zero rate turned"
            before = got
        assert counts(f) == launches(predict=K), counts(f)
        assert f.launch_info(capi.INFO_ROLES_PREDICT, 1) == cfg.roles[0]
    return got


def predict_n(cells, stream, stepwise):
    cfg, d, per = cells.cfg, cells.d, stream == "per"
    with handle(cfg, d) as f:
        f.predict_n(*imu_of(d, 0, K, per))
        got = f.get_state()
        assert counts(f) == launches(predict_n=1), counts(f)
        assert f.launch_info(capi.INFO_ROLES_PREDICT, K) == cfg.roles[1]
    cells.against_oracle(got, stream, K, f"predict_n, {stream}")
    if stepwise is not None:                                           # (the figures of test_predict_n_equals_repeated_predict)
        fig = (state_rel_err(got[0], stepwise[0], got[2])[0], cov_rel_err(got[2], stepwise[2]), cov_rel_err_blockwise(got[2], stepwise[2]))
        print(f"[edges] {cfg}: predict_n against {K} x predict, {stream}: state {fig[0]:.2e} cov {fig[1]:.2e} cov block-wise {fig[2]:.2e}")
        assert fig[0] < 2e-6 and fig[1] < 2e-6 and fig[2] < 5e-6, f"predict_n against {K} x predict, {stream}: {fig}"


def frame(cells, stream, mode, expect):
    cfg, d, per = cells.cfg, cells.d, stream == "per"
    with handle(cfg, d) as f:
        route = frame_route(f, cfg, "pose", mode, 0, K)
        assert route == expect, f"frame route {route}, expected {expect}"
        one_frame(f, d, "pose", mode, 0, K, per=per)
        got, applied = f.get_state(), f.applied()
        assert counts(f) == (launches(predict_n=1) if route == "per_call" else launches(frame=1)), (route, counts(f))
    assert (applied == 0).all()
    cells.against_oracle(got, stream, K, f"frame ({route}), {stream}")


def windows(cells, stream, mode, rows, expect, kind="pose", M=0):
    """a window of KC against the oracle and against its frames; kind / M: a measurement window of rows that name no marker"""
    cfg, d, per = cells.cfg, cells.d, stream == "per"
    what = f"{'frames' if kind == 'pose' else 'frames_meas ' + kind} ({expect}{', rows' if rows else ''}), {stream}"
    with handle(cfg, d, kind != "pose") as w, handle(cfg, d, kind != "pose") as s:
        route = window_route(w, cfg, kind, mode, M, len(KC), rows)
        assert route == expect, f"window route {route}, expected {expect}"
        traj = window(w, d, kind, mode, M, KC, rows, per=per)
        got, applied = w.get_state(), w.applied()
        k0 = 0
        for fr, k in enumerate(KC):
            one_frame(s, d, kind, mode, M, k, fr, k0, per=per)
            k0 += k
        assert counts(w) == counts(s), (counts(w), counts(s))
        frames, frames_applied = s.get_state(), s.applied()
    assert (applied == 0).all() and (frames_applied == 0).all()
    cells.against_oracle(got, stream, K, what)
    if cfg.size == "R+1" and kind == "pose":
        # past one wave per SIMD a single stacked pose frame runs frame2_kernel and the window frames_kernel: the same steps, other FMA
        # contractions (a few ulp of p and v here).  The route suite proves window == frames up to one round of waves only
        # (route_cells.CFGS), so here the frames are held to the oracle as the window is, not to the window's bits
        cells.against_oracle(frames, stream, K, f"{what}: the frames one by one")
    else:
        assert same_state(got, frames), f"{what}: the window is not its frames"
    if rows:
        nominal, pdiag, app = (t.cpu().numpy() for t in traj)
        assert (app == 0).all() and np.array_equal(nominal[-1], got[0]) and np.array_equal(pdiag[-1], np.einsum("bii->bi", got[2]))
        for fr, k in enumerate(np.cumsum(KC)):
            ref = ie.reference(cfg.nstate, cfg.dialect, stream)[k]
            cells.against_oracle((nominal[fr],) + ref[1:], stream, k, f"{what}: trajectory row {fr}")


def meas_frame(cells, stream, kind):
    cfg, d, per = cells.cfg, cells.d, stream == "per"
    with handle(cfg, d, True) as f:
        route = frame_route(f, cfg, kind, STACKED, 1, K)
        resident = cfg.dtype == 32 and f.launch_info(capi.INFO_ROLES_MEAS, 1) == 1
        assert route == ("tabled_resident" if cfg.noise else "meas_resident" if resident else "per_call"), route
        one_frame(f, d, kind, STACKED, 1, K, per=per)
        got, applied = f.get_state(), f.applied()
        assert counts(f) == (launches(predict_n=1, update=1) if route == "per_call" else launches(frame=1)), (route, counts(f))
    assert (applied == 0).all()
    cells.against_oracle(got, stream, K, f"frame_meas {kind} ({route}), {stream}")
    return route


def guard(cells, stream):
    """fp64 records: the one sample of the guard probe through predict and through the fused frame"""
    cfg, per = cells.cfg, stream == "per"
    d = data_of(cfg, guard=True)
    with handle(cfg, d) as f, handle(cfg, d) as g:
        f.predict(*imu_of(d, 0, 1, per))
        one_frame(g, d, "pose", STACKED, 0, 1, per=per)
        assert counts(g) == launches(frame=1)
        for got, what in ((f.get_state(), "predict"), (g.get_state(), "frame (f64_fused)")):
            cells.against_oracle(got, stream, 1, f"guard probe, {what}, {stream}", guard=True)


# ---- the tests -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", STATES, ids=repr)
def test_every_route_that_predicts_meets_the_gate_on_every_class(cfg):
    cells, worst = Cells(cfg), {}
    fp32 = cfg.dtype == 32
    for stream in ie.STREAMS:
        stepwise = []
        cells.run(f"predict, {stream}", lambda: stepwise.append(per_call(cells, stream, worst)))
        cells.run(f"predict_n, {stream}", lambda: predict_n(cells, stream, stepwise[0] if stepwise else None))
        cells.run(f"frame, {stream}", lambda: frame(cells, stream, STACKED, cfg.frame))
        if not fp32:
            cells.run(f"frame nearest, {stream}", lambda: frame(cells, stream, NEAREST, "per_call"))
            cells.run(f"guard probe, {stream}", lambda: guard(cells, stream))
        for rows in (False, True):
            cells.run(f"window rows {rows}, {stream}", lambda: windows(cells, stream, STACKED, rows, WINDOW_OF[cfg.frame][rows]))
        for kind in MEAS:
            cells.run(f"frame_meas {kind}, {stream}", lambda: meas_frame(cells, stream, kind))
        # the measurement windows: every kind once per handle state, rows with one stream and none with the other
        kind = MEAS[STATES.index(cfg) % 3]
        expect = "by_frame" if not fp32 else "one_wave"
        cells.run(f"frames_meas {kind}, {stream}", lambda: windows(cells, stream, STACKED, stream == "per", expect, kind, 1))
    print(f"[edges] {cfg}: worst over the samples of cell 1: " + "  ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    cells.done()


def test_graph_replay_of_the_fused_frame_equals_the_eager_run():
    """one capture, one replay, both streams"""
    cfg = next(c for c in STATES if c.name == "f32 half+1 cpp")
    d = data_of(cfg)
    for per in (False, True):
        with handle(cfg, d) as a, handle(cfg, d) as b:
            for f in (a, b):
                f.timing_enable(False)
            assert frame_route(b, cfg, "pose", STACKED, 0, K) == "fused"
            first = b.get_state()
            gid = b.graph_capture(lambda: one_frame(b, d, "pose", STACKED, 0, K, per=per))
            assert same_state(b.get_state(), first)                      # a capture records, it does not execute
            one_frame(a, d, "pose", STACKED, 0, K, per=per)
            b.graph_launch(gid)
            a.sync(); b.sync()
            assert same_state(a.get_state(), b.get_state()) and not same_state(a.get_state(), first)


def test_per_class_figures_of_the_per_call_predict():
    """every sample on its own, re-seeded from the oracle, through the per-call predict of the two plainest handle states per dialect:
    the worst figure of every class, printed (DESIGN.md section 7 records them) and held to the gate like everything else"""
    gates = dict(ie.GATES, rot=1e-5)                                   # (util.assert_parity holds the rotation to max(1e-5, 2e-6))
    for cfg in (c for c in STATES if c.name in ("f32 half+1", "f32 half+1 cpp", "f32 quarter", "f32 quarter cpp")):
        d = data_of(cfg)

        def step(state, k, per):
            with handle(cfg, d) as f:
                f.set_state(*state)                                    # (the oracle's state, rounded to the fp32 record)
                f.predict(*imu_of(d, k, k + 1, per))
                return f.get_state()
        for stream in ie.STREAMS:
            figs = ie.step_class_figures(d.scene, stream, lambda st, k: step(st, k, stream == "per"), gates)
            for c, (name, value, ratio) in sorted(figs.items()):
                print(f"[edges] {cfg}: one predict, {ie.class_name(c, stream)}: worst {name} {value:.2e} = {ratio:.2f} x gate")
            assert max(r for _, _, r in figs.values()) <= 1.0, cfg


def test_the_cells_reach_every_route_and_every_kernel_family():
    """asked of the handles, nothing launched: both route enums, the roles of predict and predict_n, the two-waves-per-SIMD forms"""
    frames, wins, families = set(), set(), set()
    for cfg in STATES:
        with handle(cfg, data_of(cfg)) as f:
            modes = (STACKED,) if cfg.dtype == 32 else (STACKED, NEAREST)
            frames.update(frame_route(f, cfg, "pose", m, 0, K) for m in modes)
            frames.update(frame_route(f, cfg, kind, STACKED, 1, K) for kind in MEAS)
            wins.update(window_route(f, cfg, "pose", STACKED, 0, len(KC), rows) for rows in (False, True))
            wins.update(window_route(f, cfg, kind, STACKED, 1, len(KC), True) for kind in MEAS)
            assert frame_route(f, cfg, "pose", STACKED, 0, K) == cfg.frame, cfg
            roles = (f.launch_info(capi.INFO_ROLES_PREDICT, 1), f.launch_info(capi.INFO_ROLES_PREDICT, K))
            assert roles == cfg.roles, (cfg, roles)
            two_wave = policy_batch(f, cfg.size) >= f.launch_info(capi.INFO_TWO_WAVE_MIN_B)
            assert two_wave == (cfg.size == "R+1"), cfg
            families.add((cfg.dtype, "predict team" if roles[0] > 1 else "predict one wave"))
            families.add((cfg.dtype, "predict_n team" if roles[1] > 1 else "predict_n parked" if two_wave or cfg.dtype == 64 else "predict_n one wave"))
            families.add((cfg.dtype, cfg.frame + (" two waves" if two_wave and cfg.frame == "fused" else "")))
    assert frames == {"per_call", "f64_fused", "fused", "team", "tabled_resident", "meas_resident"}
    assert wins == {"one_wave", "team", "team_frames", "by_frame"}
    assert families == {(32, "predict team"), (32, "predict one wave"), (64, "predict one wave"), (32, "predict_n team"),
                        (32, "predict_n one wave"), (32, "predict_n parked"), (64, "predict_n parked"), (32, "fused"),
                        (32, "fused two waves"), (32, "team"), (32, "tabled_resident"), (64, "f64_fused")}
    for dialect in (0, 1):
        for n in (18, 15):
            assert any(c.dialect == dialect and c.nstate == n and c.frame == r for c in STATES for r in ("team", "fused")), (dialect, n)
