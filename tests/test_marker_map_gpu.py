"""GPU suite: the whole marker map and odd marker counts on every update route.

Every measurement update turns a marker id into a map slot and the slot into map constants, from tables the kernels copy to LDS by hand.
That copy is written out five times, each with its own "last round is partly empty" clamp, and until this module no GPU test left the
first 16 slots or the ids 0..15.  Which test guards which copy (tests/marker_maps.py explains the ids and slots; B = 129 everywhere:
two full tiles and a last tile with ONE live lane):

  MarkerTableRegs (ekf_kernels.hpp; correct_kernel, the one-wave frame kernels, 64 threads: two rounds of id pieces split at id 512,
      fp64 mk two rounds split between slots 15 | 16)      relabel: correct *, frames one-wave, tabled; parity: pose rows
  the MAP_LATE loop of the fp64 fused frame (frame2_kernel<double>; copied behind the predict loop with stride = the live lanes of
      the tile: 1 in the last tile, whose one lane copies both tables alone)
                                                           relabel: "f64 frame fused", "f64 frames rows" (filter 128 folds a slot >= 26)
  role 3 of frames_team_kernel (ekf_team.hpp)              relabel: "frame team", "frames team *"; parity: frame K = 0 team
  MEAS_MAP_LOAD / MEAS_MAP_STORE (ekf_meas.hpp; 64, 128 or 256 threads: mkc pieces 64 and 128 lie inside slots 12 and 25, pieces
      130..159 -- slots 26..31 -- in the last, partly empty round)
                                                           relabel and parity: pixels *, corners *, frame_meas, frames_meas
  frame_kernel's lookup in global memory, with its own range test
                                                           relabel: "frame one-wave"; parity: frame K = 0 one-wave

and which the ends of the marker loops:

  for (i = role; i < M; i += NR) with the clamped prefetch (i + NR < M ? i + NR : M - 1) of correct_pixels2_kernel,
      correct_corners2_kernel and correct_pixels_split_kernel: M = 1, 2, 3, 5, 7 against 2 and 4 roles -- M below the role count (a role
      that fetches slot M - 1 and must fold nothing), M = NR + 1 (one role with a second round), M odd; M = 16 the full stride
                                                           parity: pixels, corners; padding: M = 3, 5, 7 -> 8, 13 -> 16
  MarkerGroup::fetch (groups of four; 16-byte vector path when M % 4 == 0, else the clamped scalar path with n = last - i0):
      M = 1, 3 (one partial group), 5, 6, 7 (a second group with 1, 2, 3 slots), 13 (a fourth with 1), 16 (vector path)
                                                           parity: pose rows; padding: scalar path against vector path, bit for bit

The relabelling and padding tests are exact (np.array_equal): a lost piece of a table or a slot folded twice changes a result by whole
markers.  The parity tests hold every count to the fp64 oracle with the gates of tests/util.py, imported and not restated.
M = 17 is refused by every form of the three updates with status 1 and unchanged records: tests/test_entry_forms_gpu.py asserts it.
"""
import types

import numpy as np
import pytest
import torch

import marker_maps as mm
import oracle_capi as oc
import support
from fbus_ekf import BatchedFilter, capi, noise
from util import COV_BLOCK_TOL, COV_BLOCK_TOL_F64, COV_TOL, F64_TOL, PLAIN_TOL, STATE_TOL, assert_parity, parity_errors

pytestmark = pytest.mark.gpu
STACKED, NEAREST = capi.MODE_STACKED, capi.MODE_NEAREST
C3D, TRI = capi.VIS_CORNERS3D, capi.VIS_REFRACTIVE
SPLIT0 = {"FBUS_MEAS_SPLIT": "0"}
KC = (2, 0, 1)                              # IMU samples in front of each frame of a window: unequal, one frame without any


# ---- handles and calls --------------------------------------------------------------------------------------------------------------------
def _handle(s, dtype=32, team=None, env=None, table=False, resident=False, state=None):
    """a handle on the scene's map and state; env: read once, at create; table: a per-filter noise table (five distinct rows,
    round-robin); resident: the policy batch above half a chip, where a tabled handle takes the resident window kernels"""
    with support.env(**(env or {})):
        f = BatchedFilter(s.B, s.prm, device=0, dtype=dtype, nstate=s.nstate)
    f.set_state(*(state or s.state))
    if team is not None:
        f.set_team(*team)
    if resident:
        f.set_policy_batch(64 * (f.launch_info(capi.INFO_SIMDS) // 2 + 1))
    if table:
        fact = np.array([0.3, 0.5, 1.0, 2.0, 3.0])
        f.set_noise(noise.row_of(s.prm)[None, :] * fact[(np.arange(s.B)[:, None] + 2 * np.arange(7)[None, :]) % 5])
        assert f.launch_info(capi.INFO_NOISE_RESIDENT) == int(resident and dtype == 32)
    return f


def _dev(a, f=None):
    a = np.ascontiguousarray(a)
    if a.dtype.kind in "iu":
        return torch.from_numpy(a).cuda()
    return torch.from_numpy(a.astype(f.np_dtype)).cuda()


def _imu(f, s, K):
    return (_dev(s.acc[:K], f), _dev(s.gyr[:K], f), _dev(s.dt[:K], f)) if K else (None, None, None)


def _rows(s, what, frame=None):
    """(ids, a, b) of the update `what` -- pose | left | stereo | c3d | tri -- of one frame, or of every frame of a pose scene"""
    if what == "pose":
        return (s.ids, s.pos, s.quat) if frame is None else (s.ids[frame], s.pos[frame], s.quat[frame])
    return s.ids, (s.c3 if what == "c3d" else s.left), (None if what in ("left", "c3d") else s.right)


def _update(f, s, what, mode=STACKED, nis=False):
    """one per-call update through the host-pointer entry points; returns (nis, dof) where asked"""
    ids, a, b = _rows(s, what, 0)
    if what == "pose":
        return (f.correct_nis if nis else f.correct)(ids, a, b, mode)
    if what in ("left", "stereo"):
        return (f.correct_pixels_nis if nis else f.correct_pixels)(ids, a, b)
    return (f.correct_corners_nis if nis else f.correct_corners)(ids, a, b, C3D if what == "c3d" else TRI, mode)


def _frame(f, s, what, mode=STACKED, K=0):
    """one camera frame through the fused entry points (device arrays): K predicts and the update"""
    ids, a, b = _rows(s, what, 0)
    d = (_dev(ids), _dev(a, f), None if b is None else _dev(b, f))
    if what == "pose":
        f.frame(*_imu(f, s, K), *d, mode, fused=True)
    else:
        kind, geo = (capi.MEAS_PIXELS, TRI) if what in ("left", "stereo") else (capi.MEAS_CORNERS, C3D if what == "c3d" else TRI)
        f.frame_meas(*_imu(f, s, K), *d, kind, geo, mode)
    f.sync()


def _window(f, s, what, mode=STACKED, record=False):
    """a window of len(KC) frames; the measurement rows of a one-frame scene are those of frame 0 scaled by 1 + 1e-4 per frame, so
    that no two frames are the same call"""
    if what == "pose":
        ids, a, b = _rows(s, what)
    else:
        i0, a0, b0 = _rows(s, what, 0)
        F = len(KC)
        ids = np.stack([i0] * F)
        a = mm.r32(np.stack([a0 * (1 + 1e-4 * k) for k in range(F)]))
        b = None if b0 is None else mm.r32(np.stack([b0 * (1 + 1e-4 * k) for k in range(F)]))
    d = (_dev(ids), _dev(a, f), None if b is None else _dev(b, f))
    if what == "pose":
        out = f.frames(KC, *_imu(f, s, sum(KC)), *d, mode, record=record)
    else:
        kind, geo = (capi.MEAS_PIXELS, TRI) if what in ("left", "stereo") else (capi.MEAS_CORNERS, C3D if what == "c3d" else TRI)
        out = f.frames_meas(KC, *_imu(f, s, sum(KC)), *d, kind, geo, mode, record=record)
    f.sync()
    return None if out is None else tuple(o.cpu().numpy() for o in out)


def _result(f, extra=None):
    return f.get_state(), f.applied(), () if extra is None else tuple(np.asarray(x) for x in extra)


def _assert_same(a, b, what, rename=None):
    """records, flags and whatever else the call returned: equal bit for bit (prev_id through the twin's renaming)"""
    (sa, oka, xa), (sb, okb, xb) = a, b
    for name, x, y in zip(("nominal", "rot", "P"), sa, sb):
        assert np.isfinite(np.asarray(x, np.float64)).all(), (what, name)
        if not np.array_equal(x, y):
            d = (np.asarray(x) != np.asarray(y)).reshape(len(x), -1).any(axis=1)
            raise AssertionError(f"{what}: {name} differs on {int(d.sum())} filters (first {np.nonzero(d)[0][:8]}), max |diff| "
                                 f"{np.abs(np.asarray(x, np.float64) - np.asarray(y, np.float64)).max():.3e}")
    assert np.array_equal(sa[3] if rename is None else rename(sa[3]), sb[3]), (what, "prev_id")
    assert np.array_equal(oka, okb), (what, "applied")
    assert len(xa) == len(xb) and all(np.array_equal(x, y) for x, y in zip(xa, xb)), (what, "outputs")


# ---- a. relabelling the map changes nothing, bit for bit ----------------------------------------------------------------------------------------
# (name, what, scene arguments, handle arguments, call)
def _c(mode=STACKED, nis=False):
    return lambda f, s, w: _update(f, s, w, mode, nis)


def _fr(mode=STACKED, K=2):
    return lambda f, s, w: _frame(f, s, w, mode, K)


def _w(mode=STACKED, record=False):
    return lambda f, s, w: _window(f, s, w, mode, record)


RELABEL = []
for _d in (0, 1):
    for _mode, _mn in ((STACKED, "stacked"), (NEAREST, "nearest")):
        for _t in (32, 64):
            RELABEL.append((f"correct {_mn} d{_d} f{_t}", "pose", dict(dialect=_d), dict(dtype=_t, team=(1, 1) if _t == 32 else None), _c(_mode)))
        RELABEL.append((f"correct team(1,3) {_mn} d{_d}", "pose", dict(dialect=_d), dict(team=(1, 3)), _c(_mode)))
        RELABEL.append((f"frame one-wave {_mn} d{_d}", "pose", dict(dialect=_d), dict(team=(1, 1)), _fr(_mode)))
        RELABEL.append((f"frame team {_mn} d{_d}", "pose", dict(dialect=_d), dict(team=(4, 1)), _fr(_mode)))
    for _rec in (False, True):
        _r = " rows" if _rec else ""
        RELABEL.append((f"frames one-wave{_r} d{_d}", "pose", dict(dialect=_d), dict(team=(1, 1)), _w(NEAREST if _d else STACKED, _rec)))
        RELABEL.append((f"frames team{_r} d{_d}", "pose", dict(dialect=_d), dict(team=(4, 1)), _w(NEAREST if _d else STACKED, _rec)))
    RELABEL.append((f"f64 frame fused d{_d}", "pose", dict(dialect=_d), dict(dtype=64), _fr(STACKED)))
    RELABEL.append((f"f64 frames rows d{_d}", "pose", dict(dialect=_d), dict(dtype=64), _w(STACKED, True)))
    RELABEL.append((f"tabled correct d{_d}", "pose", dict(dialect=_d), dict(table=True), _c(NEAREST if _d else STACKED)))
    RELABEL.append((f"tabled resident frames d{_d}", "pose", dict(dialect=_d), dict(table=True, resident=True), _w(STACKED, True)))
RELABEL.append(("correct stacked n15", "pose", dict(dialect=1, nstate=15), dict(team=(1, 1)), _c(STACKED)))
for _k in ("left", "stereo"):
    RELABEL += [(f"pixels {_k} one-wave", _k, {}, dict(team=(0, 1)), _c()),
                (f"pixels {_k} split", _k, {}, {}, _c()),
                (f"pixels {_k} set_team(0,2)", _k, {}, dict(team=(0, 2)), _c()),
                (f"pixels {_k} one-tail 2 roles", _k, {}, dict(team=(0, 2), env=SPLIT0), _c()),
                (f"pixels {_k} one-tail 4 roles", _k, {}, dict(env=SPLIT0), _c()),
                (f"pixels {_k} f64", _k, {}, dict(dtype=64), _c()),
                (f"pixels {_k} f64 one role", _k, {}, dict(dtype=64, team=(0, 1)), _c()),
                (f"pixels {_k} nis", _k, {}, {}, _c(nis=True)),
                (f"frame_meas {_k}", _k, {}, dict(team=(1, 1)), _fr(K=2)),
                (f"frames_meas {_k} rows", _k, {}, dict(team=(1, 1)), _w(record=True))]
for _k in ("c3d", "tri"):
    RELABEL += [(f"corners {_k} stacked", _k, dict(dialect=1), {}, _c(STACKED)),
                (f"corners {_k} nearest", _k, dict(dialect=1), {}, _c(NEAREST)),
                (f"corners {_k} nearest matlab f64", _k, dict(dialect=0), dict(dtype=64), _c(NEAREST)),
                (f"frame_meas corners {_k} nearest", _k, dict(dialect=1), dict(team=(1, 1)), _fr(NEAREST, 2))]


@pytest.mark.parametrize("name,what,sargs,hargs,call", RELABEL, ids=[c[0] for c in RELABEL])
def test_relabelling_the_map_changes_nothing(name, what, sargs, hargs, call):
    """The M = 5 scene on the full map and on its twin -- the same 32 markers in other slots under other ids, 0 and 1023 on other markers:
    records, flags, NIS and trajectory rows equal bit for bit (prev_id: renamed).  A copy of the id table or of the map constants that
    misses a piece makes the two runs differ by whole markers."""
    s = mm.pose_scene(M=5, frames=3, **sargs) if what == "pose" else mm.meas_scene(M=5, **sargs)
    t = mm.twin_of(s)
    out = []
    for scene in (s, t):
        with _handle(scene, **hargs) as f:
            extra = call(f, scene, what)
            out.append(_result(f, extra))
    assert out[0][1].sum() >= mm.B - 2 and not np.array_equal(out[0][0][0], s.state[0].astype(out[0][0][0].dtype))
    _assert_same(out[0], out[1], name, t.rename)


# ---- b. parity with the fp64 oracle at every marker count -----------------------------------------------------------------------------------------
def _gates(e, dtype, what, cov_block64=COV_BLOCK_TOL_F64):
    """the single-step gates of tests/util.py on the figures e = parity_errors(got, oracle)"""
    if dtype == 64:
        assert e["literal"] < F64_TOL and e["sigma"] < F64_TOL and e["plain"] < F64_TOL and e["cov"] < F64_TOL, (what, e)
        assert e["cov_block"] < cov_block64, (what, e["cov_block"])
    else:
        assert e["literal"] <= STATE_TOL and e["sigma"] <= STATE_TOL and e["plain"] <= PLAIN_TOL, (what, e)
        assert e["cov"] <= COV_TOL and e["cov_block"] <= COV_BLOCK_TOL, (what, e)
    assert e["asym"] == 0 and e["prev_equal"], what


def _line(what, e):
    print(f"[parity] {what}: literal {e['literal']:.2e}  sigma-aware {e['sigma']:.2e} ({e['sigma_block']})  plain per-block "
          f"{e['plain']:.2e} ({e['plain_block']})  cov {e['cov']:.2e}  cov block-wise {e['cov_block']:.2e}")


class _Worst:
    """the worst figure of a case, per record type, printed behind it ([worst] lines: the "measured" comments come from them)"""

    def __init__(self, what):
        self.what, self.w = what, {}

    def add(self, dtype, e):
        w = self.w.setdefault(dtype, dict.fromkeys(("literal", "sigma", "plain", "cov", "cov_block"), 0.0))
        for k in w:
            w[k] = max(w[k], e[k])

    def show(self):
        for dtype, w in sorted(self.w.items()):
            print(f"[worst] {self.what} fp{dtype}: " + "  ".join(f"{k} {v:.2e}" for k, v in w.items()))


@pytest.mark.parametrize("dialect", [0, 1])
@pytest.mark.parametrize("mode", [STACKED, NEAREST])
@pytest.mark.parametrize("M", mm.POSE_M)
def test_pose_rows_match_the_oracle_at_every_marker_count(M, mode, dialect):
    """One update per handle; correct on the one-wave kernel and with set_team(1, 3), both record types, and the fused frame with K = 0 on
    the one-wave route (frame_kernel: the lookup in global memory) and on the team route.
    measured (MI355X), worst over the routes, M = 1 | 3 | 5 | 6 | 7 | 13 | 16, fp32: literal 3.2e-07 | 4.8e-07 | 5.2e-07 | 5.4e-07 | 5.6e-07 |
    7.3e-07 | 6.9e-07, sigma-aware 3.9e-07 .. 9.7e-07, plain 1.2e-05 .. 4.2e-05, cov <= 2.0e-07, cov block-wise 2.1e-07 | 3.6e-07 | 3.3e-07 |
    4.8e-07 | 4.2e-07 | 7.4e-07 | 7.8e-07; fp64: literal <= 9.8e-16, plain <= 5.6e-14, cov block-wise <= 2.1e-15"""
    s = mm.pose_scene(M=M, dialect=dialect)
    want, ok = mm.oracle_update(s, "pose", mode)
    assert ok.all()
    worst = _Worst(f"pose rows M {M} {'stacked' if mode else 'nearest'} d{dialect}")
    for dtype, team, fused in ((32, (1, 1), False), (32, (1, 3), False), (64, None, False), (64, (1, 3), False),
                               (32, (1, 1), True), (32, (4, 1), True)):
        with _handle(s, dtype=dtype, team=team) as f:
            if fused:
                _frame(f, s, "pose", mode, 0)
            else:
                _update(f, s, "pose", mode)
            got, app = f.get_state(), f.applied()
        what = f"{worst.what} fp{dtype} set_team{team} {'frame K = 0' if fused else 'correct'}"
        e = parity_errors(got, want)
        _line(what, e)
        worst.add(dtype, e)
        assert np.array_equal(app, ok), what
        assert_parity(got, want, dtype, what, verbose=False)
    worst.show()


PIXEL_ROUTES = (  # name, record type, set_team, environment, form, (INFO_MEAS_SPLIT, INFO_ROLES_MEAS) expected for M >= 2
    ("one-wave", 32, (0, 1), None, "call", (0, 1)), ("split", 32, None, None, "call", (4, 4)), ("set_team(0,2)", 32, (0, 2), None, "call", (2, 2)),
    ("one-tail 2 roles", 32, (0, 2), SPLIT0, "call", (0, 2)), ("one-tail 4 roles", 32, None, SPLIT0, "call", (0, 4)),
    ("f64", 64, None, None, "call", (0, 4)), ("f64 one role", 64, (0, 1), None, "call", (0, 1)), ("nis", 32, None, None, "nis", None),
    ("frame_meas K = 0", 32, (1, 1), None, "frame", (0, 1)))


@pytest.mark.parametrize("kind", ["left", "stereo"])
@pytest.mark.parametrize("M", mm.PIXEL_M)
def test_pixel_rows_match_the_oracle_at_every_marker_count(M, kind):
    """correct_pixels on every route, correct_pixels_nis and frame_meas with K = 0 against the analytic oracle in both covariance forms.
    fp64: F64_TOL; the block-wise covariance against the oracle's LITERAL (I - K H) P gets 1e-6, as test_correct_pixels_matches_the_oracle
    explains (the oracle's form cancels there), against its Joseph form F64_TOL.  M = 1 takes the one-wave kernel on every setting.
    measured (MI355X), worst over the routes, M = 1 | 2 | 3 | 5 | 7 | 16, fp32 (the same against both forms): literal 5.3e-08 | 5.7e-08 |
    6.0e-08 | 7.5e-08 | 5.3e-08 | 6.1e-08, sigma-aware <= 9.7e-08, plain <= 5.2e-07, cov <= 5.7e-08, cov block-wise 1.9e-07 | 2.5e-07 |
    2.8e-07 | 2.7e-07 | 2.7e-07 | 2.5e-07; fp64: literal 7.0e-13 | 2.2e-12 | 4.0e-12 | 5.9e-12 | 4.9e-12 | 6.7e-12, plain <= 1.3e-10, cov
    block-wise against the Joseph form 8.4e-13 .. 9.6e-12, against the literal form 9.8e-12 | 1.7e-10 | 1.1e-09 | 2.1e-09 | 1.5e-08 | 8.0e-08"""
    s = mm.meas_scene(M=M)
    want = {form: mm.oracle_update(s, kind, cov_form=form) for form in (oc.SIMPLE, oc.JOSEPH)}
    ok = want[oc.SIMPLE][1]
    assert ok.all() and np.array_equal(ok, want[oc.JOSEPH][1])
    worst = {form: _Worst(f"pixel rows M {M} {kind} vs {'Joseph' if form else 'simple'}-form oracle") for form in want}
    for name, dtype, team, env, form, info in PIXEL_ROUTES:
        with _handle(s, dtype=dtype, team=team, env=env) as f:
            if M == 1:
                assert f.launch_info(capi.INFO_MEAS_SPLIT, 1) == 0 and f.launch_info(capi.INFO_ROLES_MEAS, 1) == 1
            elif info is not None:
                assert (f.launch_info(capi.INFO_MEAS_SPLIT, M), f.launch_info(capi.INFO_ROLES_MEAS, M)) == info, name
            if form == "frame":
                _frame(f, s, kind)
            else:
                _update(f, s, kind, nis=form == "nis")
            got, app = f.get_state(), f.applied()
        assert np.array_equal(app, ok), name
        for cf, (ref, _) in want.items():
            what = f"{worst[cf].what} fp{dtype} {name}"
            e = parity_errors(got, ref)
            _line(what, e)
            worst[cf].add(dtype, e)
            _gates(e, dtype, what, cov_block64=F64_TOL if cf == oc.JOSEPH else 1e-6)
    for w in worst.values():
        w.show()


@pytest.mark.parametrize("dialect", [0, 1])
@pytest.mark.parametrize("geometry", ["c3d", "tri"])
@pytest.mark.parametrize("M", mm.CORNER_M)
def test_corner_rows_match_the_oracle_at_every_marker_count(M, geometry, dialect):
    """correct_corners, the corners themselves and triangulated through the port: stacked with one, two and four roles, nearest (C++
    dialect: with hysteresis), both record types; frame_meas with K = 0.  fp64 at F64_TOL, block-wise covariance included.
    measured (MI355X), worst over the routes, M = 1 | 3 | 5 | 7, fp32: literal 5.2e-08 | 5.4e-08 | 5.6e-08 | 5.2e-08, sigma-aware <= 9.0e-08,
    plain <= 5.1e-07, cov <= 5.6e-08, cov block-wise 1.8e-07 | 2.1e-07 | 2.4e-07 | 2.3e-07; fp64: literal <= 3.1e-14, plain <= 9.8e-13,
    cov block-wise <= 3.6e-15"""
    s = mm.meas_scene(M=M, dialect=dialect)
    worst = _Worst(f"corner rows M {M} {geometry} d{dialect}")
    for mode in (STACKED, NEAREST):
        want, ok = mm.oracle_update(s, geometry, mode)
        assert ok.all()
        for dtype, team, fused in ((32, (0, 1), False), (32, (0, 2), False), (32, (0, 4), False), (64, None, False), (64, (0, 1), False),
                                   (32, (1, 1), True)):
            if mode == NEAREST and team in ((0, 2), (0, 4)):
                continue                                    # (the nearest mode has one kernel)
            with _handle(s, dtype=dtype, team=team) as f:
                if mode == STACKED and M >= 2 and not fused:
                    assert f.launch_info(capi.INFO_ROLES_MEAS, M) == (4 if team is None else team[1])
                if fused:
                    _frame(f, s, geometry, mode)
                else:
                    _update(f, s, geometry, mode)
                got, app = f.get_state(), f.applied()
            what = f"{worst.what} {'stacked' if mode else 'nearest'} fp{dtype} set_team{team}{' frame_meas K = 0' if fused else ''}"
            e = parity_errors(got, want)
            _line(what, e)
            worst.add(dtype, e)
            assert np.array_equal(app, ok), what
            _gates(e, dtype, what, cov_block64=F64_TOL)
    worst.show()


# ---- c. padding to a larger M changes nothing, bit for bit ------------------------------------------------------------------------------------------
def _padded(s, Mp):
    """the scene with Mp slots per filter: the trailing ones absent (-1), NaN in their image points, corners and poses"""
    t = types.SimpleNamespace(**vars(s))
    t.M = Mp

    def pad(a, fill):
        a = np.asarray(a)
        ax = 2 if s.kind == "pose" else 1                   # (F, B, M, ...) | (B, M, ...)
        shape = list(a.shape)
        shape[ax] = Mp - s.M
        return np.concatenate([a, np.full(shape, fill, a.dtype)], axis=ax)
    t.ids = pad(s.ids, -1)
    for name in ("pos", "quat") if s.kind == "pose" else ("left", "right", "c3"):
        setattr(t, name, pad(getattr(s, name), np.nan))
    return t


@pytest.mark.parametrize("mode", [STACKED, NEAREST])
@pytest.mark.parametrize("M,Mp", mm.PAD)
def test_padding_the_pose_rows_changes_nothing(M, Mp, mode):
    """M = 3, 5, 7 as they are and padded to 8, M = 13 padded to 16: the padded call takes MarkerGroup::fetch's 16-byte vector path, the
    unpadded one its clamped scalar path -- they load the same values.  One-wave, set_team(1, 3), fp64; the fused frame on both routes."""
    for dialect in (0, 1):
        s = mm.pose_scene(M=M, dialect=dialect)
        p = _padded(s, Mp)
        for dtype, team, fused in ((32, (1, 1), False), (32, (1, 3), False), (64, None, False), (32, (1, 1), True), (32, (4, 1), True)):
            out = []
            for scene in (s, p):
                with _handle(scene, dtype=dtype, team=team) as f:
                    if fused:
                        _frame(f, scene, "pose", mode, 2)
                    else:
                        _update(f, scene, "pose", mode)
                    out.append(_result(f))
            assert out[0][1].all()
            _assert_same(out[0], out[1], f"pose rows M {M} -> {Mp} mode {mode} d{dialect} fp{dtype} set_team{team}{' frame' if fused else ''}")


PAD_ROUTES = (("one-wave", 32, (0, 1), None, (0, 1)), ("2 roles", 32, (0, 2), SPLIT0, (0, 2)), ("4 roles", 32, (0, 4), SPLIT0, (0, 4)),
              ("split 2", 32, None, {"FBUS_MEAS_SPLIT": "2"}, (2, None)), ("split 4", 32, None, {"FBUS_MEAS_SPLIT": "4"}, (4, None)),
              ("f64", 64, None, None, (0, 4)))


@pytest.mark.parametrize("what", ["left", "stereo", "c3d", "tri"])
@pytest.mark.parametrize("M,Mp", mm.PAD)
def test_padding_the_measurement_rows_changes_nothing(M, Mp, what):
    """The same for the pixel and corner rows, between handles pinned to the same role count: one wave, two and four roles, the split
    kernel with two and four waves, fp64.  The roles walk the slots with stride NR: the padded call gives some of them a further round
    of absent slots, which must fold nothing."""
    s = mm.meas_scene(M=M)
    p = _padded(s, Mp)
    for name, dtype, team, env, info in PAD_ROUTES:
        if what in ("c3d", "tri") and name.startswith("split"):
            continue                                        # (the split kernel is the pixel rows')
        out = []
        for scene in (s, p):
            with _handle(scene, dtype=dtype, team=team, env=env) as f:
                if what in ("left", "stereo"):
                    assert f.launch_info(capi.INFO_MEAS_SPLIT, scene.M) == info[0], name
                if info[1] is not None:
                    assert f.launch_info(capi.INFO_ROLES_MEAS, scene.M) == info[1], name
                _update(f, scene, what)
                out.append(_result(f))
        assert out[0][1].all()
        _assert_same(out[0], out[1], f"{what} M {M} -> {Mp} {name}")


# ---- d. hysteresis with large ids -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [32, 64])
@pytest.mark.parametrize("what", ["pose", "c3d", "tri"])
def test_hysteresis_carries_large_ids(what, dtype):
    """C++ dialect, nearest mode, two consecutive updates on the full map: the previous marker keeps its place on some filters and loses it
    on others (tests/test_marker_map_cpu.py counts both on these scenes), prev_id equals the oracle's exactly after each update -- id
    1023 travels through the fp32 record -- and the second update, re-seeded from the first one's records, meets the single-step gates.
    measured (MI355X), second update, fp32: pose rows literal 1.8e-07, sigma-aware 1.8e-07, plain 4.1e-06, cov block-wise 2.5e-07; corners
    through the port literal 4.8e-08, sigma-aware 8.3e-08, cov block-wise 2.0e-07; fp64: literal <= 1.3e-14, cov block-wise <= 5.9e-16"""
    s = mm.pose_scene(M=5, dialect=1, frames=3) if what == "pose" else mm.meas_scene(M=5, dialect=1)
    second = types.SimpleNamespace(**vars(s))
    if what == "pose":
        second.ids, second.pos, second.quat = s.ids[1:], s.pos[1:], s.quat[1:]
    else:                                                   # the same view a moment later: other slot order, the image points moved by noise
        rng = np.random.default_rng(5)
        second.ids = np.ascontiguousarray(s.ids[:, ::-1])
        second.c3 = mm.r32(s.c3[:, ::-1] + rng.normal(0, 0.002, s.c3.shape))
        second.left = mm.r32(s.left[:, ::-1] + rng.normal(0, 3e-4, s.left.shape))
        second.right = mm.r32(s.right[:, ::-1] + rng.normal(0, 3e-4, s.right.shape))
    want1, ok1 = mm.oracle_update(s, what, NEAREST)
    with _handle(s, dtype=dtype) as f:
        _update(f, s, what, NEAREST)
        got1, app1 = f.get_state(), f.applied()
        if what != "pose":                                  # the marker just taken leaves the view of every third filter
            taken = got1[3]
            gone = (second.ids == taken[:, None]) & (np.arange(s.B) % 3 == 0)[:, None]
            second.ids = np.where(gone, -1, second.ids).astype(np.int32)
        _update(f, second, what, NEAREST)
        got2, app2 = f.get_state(), f.applied()
    assert np.array_equal(app1, ok1) and ok1.all() and np.array_equal(got1[3], want1[3])
    assert (got1[3] == 1023).any() and (got1[3] != s.state[3]).any() and (got1[3] == s.state[3]).any()
    assert_parity(got1, want1, dtype, f"hysteresis {what} fp{dtype}, first update")
    seed = tuple(np.asarray(x, np.float64) if x.dtype.kind == "f" else x for x in got1)
    want2, ok2 = mm.oracle_update(second, what, NEAREST, state=seed)
    assert np.array_equal(app2, ok2) and ok2.all() and np.array_equal(got2[3], want2[3])
    changed = (got2[3] != got1[3]).sum()
    print(f"[hysteresis] {what} fp{dtype}: second update changes the marker on {changed} of {s.B} filters")
    assert changed >= 4 and (what == "pose" or changed <= s.B - 4)    # (pose rows: frame 1 shows other markers, few can keep theirs)
    assert_parity(got2, want2, dtype, f"hysteresis {what} fp{dtype}, second update")
