"""CPU suite: the fixtures of tests/marker_maps.py are what they claim, before tests/test_marker_map_gpu.py relies on them.
The full map validates and holds the boundary ids where stated; every scene the GPU module runs reaches the slots and ids at the round
boundaries of the kernels' map copies (marker_maps.py's docstring lists which copy each one is there for); the oracle does not see
labels; and its two pixel oracles agree on the largest scene."""
import ctypes as C

import numpy as np
import pytest

import marker_maps as mm
import oracle_capi as oc
from fbus_ekf import capi
from util import parity_errors

MODES = (capi.MODE_STACKED, capi.MODE_NEAREST)


def test_the_full_map_is_valid_and_holds_the_boundary_ids():
    lib = capi.load_library()
    msg = C.create_string_buffer(256)
    for dialect in (0, 1):
        prm = mm.params(dialect)
        assert lib.fbus_params_validate(C.byref(prm), msg, 256) == 0, msg.value
        ids, pos, rot = mm.read_map(prm)
        assert prm.n_markers == capi.MAX_MARKERS == 32 and prm.marker_size == mm.SIZE
        assert len(set(ids)) == 32 and set(mm.EDGE_IDS) <= set(int(i) for i in ids) and ids.min() == 0 and ids.max() == 1023
        assert ids[0] == 1023 and ids[31] == 0 and list(ids) != sorted(ids)
        assert {int(ids[s]) for s in mm.EDGE_SLOTS} == set(mm.EDGE_IDS)
        # no two slots share a position or an orientation, and every rotation is one
        assert len({tuple(np.round(p, 9)) for p in pos}) == 32 and len({tuple(np.round(r.ravel(), 9)) for r in rot}) == 32
        assert np.abs(rot @ np.swapaxes(rot, 1, 2) - np.eye(3)).max() < 1e-12
        # the twin: the same markers, no slot and no boundary label kept
        twin = capi.FbusParams.from_buffer_copy(prm)
        eng = mm.oracle_engine(mm.pose_scene(M=5, dialect=dialect), batch=1)
        out = mm.relabel(twin, eng.orc.prm, np.array([[1023, 0, -1, 7]], np.int32), seed=mm.TWIN_SEED)
        assert lib.fbus_params_validate(C.byref(twin), msg, 256) == 0, msg.value
        tids, tpos, trot = mm.read_map(twin)
        assert set(int(i) for i in tids) == set(mm.TWIN_IDS) and {0, 1023} <= set(int(i) for i in tids)
        assert list(eng.orc.prm.marker_id)[:32] == list(tids)
        where = {tuple(np.round(p, 9)): k for k, p in enumerate(pos)}
        back = np.array([where[tuple(np.round(p, 9))] for p in tpos])                 # the old slot of every new slot
        assert sorted(back) == list(range(32)) and (back != np.arange(32)).all()
        assert np.array_equal(trot, rot[back])
        assert not np.isin(ids[back][np.isin(tids, (0, 1023))], (0, 1023)).any()
        assert out[0, 2] == -1 and tids[list(back).index(0)] == out[0, 0] and tids[list(back).index(31)] == out[0, 1]


def _frames_of(scene):
    return [scene.ids[f] for f in range(scene.ids.shape[0])] if scene.kind == "pose" else [scene.ids]


def _assert_coverage(ids2d, M, what, prm=None):
    per_slot, per_id, last = mm.coverage(ids2d, prm)
    table = [int(i) for i in (mm.IDS if prm is None else mm.read_map(prm)[0])]
    assert ids2d.shape == (mm.B, M)
    for s in mm.EDGE_SLOTS:
        assert per_slot[s] >= 4, (what, "slot", s, per_slot[s])
    for i in mm.EDGE_IDS:
        if i in table:
            assert per_id[i] >= 4, (what, "id", i, per_id[i])
    assert max(last) >= 26, (what, "filter 128 folds slots", last)
    full = (ids2d >= 0).all(axis=1).sum()
    assert full >= mm.B / 4, (what, "filters with all slots", full)
    if M >= 3:
        assert ((ids2d < 0).any(axis=1)).sum() >= 4, what
    assert np.isin(ids2d[ids2d >= 0], table).all()


@pytest.mark.parametrize("dialect", [0, 1])
def test_every_scene_reaches_the_round_boundaries(dialect):
    for M in mm.POSE_M:
        s = mm.pose_scene(M=M, dialect=dialect)
        _assert_coverage(s.ids[0], M, f"pose M {M}")
        # the nearest mode never skips: every measured marker lies within 10 m
        assert np.linalg.norm(s.pos[0], axis=-1).max() < 10.0
        for a in (s.pos, s.quat) + s.state[:3]:
            assert np.array_equal(a, mm.r32(a))
    w = mm.pose_scene(M=5, dialect=dialect, frames=3)
    for f in range(3):
        _assert_coverage(w.ids[f], 5, f"pose window frame {f}")
    assert np.array_equal(w.ids[0], mm.pose_scene(M=5, dialect=dialect).ids[0])
    for M in sorted(set(mm.PIXEL_M + mm.CORNER_M + tuple(m for m, _ in mm.PAD))):
        s = mm.meas_scene(M=M, dialect=dialect)
        _assert_coverage(s.ids, M, f"pixels M {M}")
        assert np.linalg.norm(s.c3.reshape(mm.B, M, 4, 3)[s.ids >= 0], axis=-1).max() < 10.0
        for a in (s.left, s.right, s.c3) + s.state[:3]:
            assert np.array_equal(a, mm.r32(a))
    # M = 16 is filled: the view from 1.2 - 1.8 m holds at least 16 markers
    nvis = (mm.meas_scene(M=16, dialect=dialect).ids >= 0).sum(axis=1)
    assert nvis.mean() > 14 and nvis.max() == 16, nvis
    # the twins of the M = 5 scenes reach the boundaries of THEIR tables, and the padded scenes are their unpadded ones
    for s in (mm.pose_scene(M=5, dialect=dialect, frames=3), mm.meas_scene(M=5, dialect=dialect)):
        t = mm.twin_of(s)
        for ids2d in _frames_of(t):
            _assert_coverage(ids2d, 5, "twin", t.prm)
    for m, mp in mm.PAD:
        assert m in mm.POSE_M and (m in mm.PIXEL_M or m == 13)


@pytest.mark.parametrize("dialect", [0, 1])
def test_the_oracle_is_label_blind(dialect):
    """fbo_correct and fbo_correct_pixels_analytic on a scene and on its relabelled twin: bit-equal records, and prev_id renamed.  If they
    were not, the fixture would be wrong, not a kernel."""
    s = mm.pose_scene(M=5, dialect=dialect, frames=3)
    t = mm.twin_of(s)
    old, new = mm.read_map(s.prm)[0], mm.read_map(t.prm)[0]
    assert not np.array_equal(old, new) and np.array_equal(t.pos, s.pos) and not np.array_equal(t.ids, s.ids)
    for mode in MODES:
        (a, oka), (b, okb) = mm.oracle_update(s, "pose", mode), mm.oracle_update(t, "pose", mode)
        assert np.array_equal(oka, okb) and oka.all()
        assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3]))
        assert np.array_equal(mm.relabel(capi.FbusParams.from_buffer_copy(s.prm), None, a[3], mm.TWIN_SEED), b[3])
    s = mm.meas_scene(M=5, dialect=dialect)
    t = mm.twin_of(s)
    for what in ("left", "stereo", "c3d", "tri"):
        for mode in (MODES if what in ("c3d", "tri") else MODES[:1]):
            (a, oka), (b, okb) = mm.oracle_update(s, what, mode), mm.oracle_update(t, what, mode)
            assert np.array_equal(oka, okb) and oka.all()
            assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])), (what, mode)
            assert np.array_equal(mm.relabel(capi.FbusParams.from_buffer_copy(s.prm), None, a[3], mm.TWIN_SEED), b[3])


def test_the_two_pixel_oracles_agree_on_the_sixteen_marker_scene():
    """closed-form against central-difference rows on the M = 16 full-map scene, the bound of tests/test_oracle_pixels_cpu.py"""
    s = mm.meas_scene(M=16)
    for what in ("left", "stereo"):
        a, oka = mm.oracle_update(s, what, analytic=True)
        f, okf = mm.oracle_update(s, what, analytic=False)
        assert np.array_equal(oka, okf) and oka.all()
        e = parity_errors(a, f)
        print(f"[oracles] M = 16 {what}: literal {e['literal']:.2e} sigma-aware {e['sigma']:.2e} cov block-wise {e['cov_block']:.2e}")
        assert e["literal"] < 1e-7 and e["sigma"] < 1e-6 and e["cov_block"] < 1e-6


def test_the_hysteresis_scenes_keep_and_lose_the_previous_marker():
    """C++ dialect, nearest mode: the scenes of the GPU module's hysteresis test do both -- on some filters the previous marker is not
    the nearest and keeps its place, on others it loses it -- and id 1023 is among the markers taken."""
    for s, what in ((mm.pose_scene(M=5, dialect=1, frames=3), "pose"), (mm.meas_scene(M=5, dialect=1), "c3d")):
        prev = s.state[3]
        after, ok = mm.oracle_update(s, what, capi.MODE_NEAREST)
        assert ok.all()
        ids0 = s.ids[0] if what == "pose" else s.ids
        first = s.pos[0] if what == "pose" else s.c3[:, :, 0:3]
        d = np.where(ids0 >= 0, np.linalg.norm(first, axis=-1), np.inf)
        nearest = ids0[np.arange(s.B), d.argmin(axis=1)]
        seen = (ids0 == prev[:, None]).any(axis=1) & (prev != nearest)
        kept, lost = seen & (after[3] == prev), seen & (after[3] != prev)
        print(f"[hysteresis] {what}: previous marker in view and not the nearest on {seen.sum()} filters: kept on {kept.sum()}, lost on {lost.sum()}")
        assert kept.sum() >= 4 and lost.sum() >= 4 and (after[3][lost] == nearest[lost]).all()
        assert (after[3] == 1023).sum() >= 1
