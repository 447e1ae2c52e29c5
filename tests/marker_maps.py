"""Fixtures of the marker-map tests (tests/test_marker_map_cpu.py, tests/test_marker_map_gpu.py): a FULL map -- 32 markers
(FBUS_MAX_MARKERS) whose ids reach 1023 (FBUS_MAX_MARKER_ID) -- its relabelled twin, and scenes of B = 129 filters at every
marker count.  No tests here.

Why these numbers.  Every update turns a marker id into a map slot (id2slot, 1024 shorts = 128 pieces of 16 bytes, 8 ids each) and the
slot into map constants (fp32 mk: 2 pieces per slot; fp64 mk: 4 per slot, 128 in all; the measurement kernels' mkc: 5 per slot, 160 in
all).  The kernels copy both tables to LDS 16 bytes per thread and round, with 64, 128 or 256 threads:
  * ids 0 | 7 | 8: the two ends of piece 0 and the first id of piece 1; 511 | 512: the last piece of a 64-thread copy's first round
    and the first of its second (128 threads copy the table in one round, 256 leave their upper half idle); 1016 | 1023: the two
    ends of the last piece.
  * slots 12 | 25: their mkc pieces 60..64 and 125..129 straddle the rounds of a 64-thread copy (and 128-thread: 125..129); 15 | 16:
    the fp64 mk copy's pieces 60..63 | 64..67, the round boundary of a one-wave copy; 26: mkc pieces 130..134, wholly in the last,
    partly empty round; 0 and 31: the ends of every table.
A copy that drops its last round, clamps one piece too early or skips a thread's share loses exactly such an id or slot; the default
map (12 markers, ids below 32) and the 16-marker wall never touch any of them but id 0 / slot 0.

B = 129: two full 64-filter tiles and a last tile with ONE live lane (frames_kernel's fp64 copy strides by the live lanes of the
tile: nact = 1; the per-call kernels clamp 63 lanes onto the last filter).  Filter 128 is that lane.
"""
import types

import numpy as np

import oracle_capi as oc
from fbus_ekf import capi, synth
from support import frozen, r32
from util import pixel_scene

B = 129
SIZE = 0.2                                   # marker edge [m]: 0.3 m pitch leaves room for the in-plane rotation of each marker
PITCH = 0.3
EDGE_IDS = (0, 7, 8, 511, 512, 1016, 1023)
EDGE_SLOTS = (0, 12, 15, 16, 25, 26, 31)
# slot order: a fixed shuffle.  Slot 0 holds id 1023, slot 31 id 0; the other five edge slots hold the other five edge ids, so that an
# M = 1 scene (129 folds in all) can still put four filters on every one of them
IDS = (1023, 300, 64, 895, 16, 640, 127, 960, 3, 448, 768, 200, 7, 600, 255, 512,
       8, 800, 63, 384, 1000, 128, 700, 15, 896, 1016, 511, 256, 767, 100, 383, 0)
# the twin's id list: 0 and 1023 again (on other markers, relabel() sees to that), otherwise the neighbours of the boundaries above
TWIN_IDS = (0, 1023, 1, 2, 9, 10, 17, 31, 32, 65, 129, 257, 510, 513, 514, 639,
            641, 766, 769, 894, 897, 1015, 1017, 1022, 500, 501, 250, 750, 40, 80, 160, 320)
assert len(set(IDS)) == 32 and len(set(TWIN_IDS)) == 32 and set(EDGE_IDS) <= set(IDS)
assert IDS[0] == 1023 and IDS[31] == 0 and {IDS[s] for s in EDGE_SLOTS} == set(EDGE_IDS)


# ---- the map ------------------------------------------------------------------------------------------------------------------------------
def _rz(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])


def _rx(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[1.0, 0, 0], [0, c, -s], [0, s, c]])


def write_map(prm, orc_prm, ids, pos, rot):
    """the table (ids (n,), pos (n, 3), rot (n, 3, 3)) into the product's parameters and the oracle's (which holds quaternions)"""
    n = len(ids)
    prm.n_markers = n
    if orc_prm is not None:
        orc_prm.n_markers = n
    for k in range(n):
        prm.marker_id[k] = int(ids[k])
        q = synth.R2q(rot[k])
        for i in range(3):
            prm.marker_pos[k][i] = float(pos[k][i])
        for i in range(9):
            prm.marker_rot[k][i] = float(rot[k].ravel()[i])
        if orc_prm is not None:
            orc_prm.marker_id[k] = int(ids[k])
            for i in range(3):
                orc_prm.marker_pos[k][i] = float(pos[k][i])
            for i in range(4):
                orc_prm.marker_quat[k][i] = float(q[i])


def read_map(prm):
    n = prm.n_markers
    return (np.array(list(prm.marker_id)[:n], np.int32), np.array([list(prm.marker_pos[k]) for k in range(n)], float),
            np.array([list(prm.marker_rot[k]) for k in range(n)], float).reshape(n, 3, 3))


def full_map(prm, orc_prm, size):
    """A wall of 8 x 4 = 32 markers at 0.3 m pitch around the default map's marker 0, in its plane, every marker turned by its own few
    degrees in the plane and out of it (no two slots share a constant), ids IDS in slot order; into the product's parameters and the
    oracle's (None: the product's alone).  Sets marker_size."""
    _, mpos, _ = synth.marker_table(prm)
    R0 = np.array(list(prm.marker_rot[0])).reshape(3, 3)
    p0 = mpos[0].copy()
    pos, rot = np.zeros((32, 3)), np.zeros((32, 3, 3))
    for k in range(32):
        pos[k] = p0 + R0 @ np.array([PITCH * (k % 8 - 3.5), PITCH * (k // 8 - 1.5), 0.0])
        rot[k] = R0 @ _rz(0.006 * (k - 15.5)) @ _rx(0.004 * ((7 * k) % 32 - 15.5))
    write_map(prm, orc_prm, IDS, pos, rot)
    prm.marker_size = size


def relabel(prm, orc_prm, ids, seed):
    """The same 32 markers in other slots under other ids (TWIN_IDS; 0 and 1023 land on markers that held neither, and no marker keeps
    its slot), in place; returns the measurement id array(s) `ids` rewritten to the new names (-1 stays -1).  Physically nothing
    changes."""
    old_ids, pos, rot = read_map(prm)
    n = len(old_ids)
    assert n == 32
    rng = np.random.default_rng(seed)
    while True:
        perm = rng.permutation(n)                       # new slot j holds the marker of old slot perm[j]
        new_ids = np.array(TWIN_IDS, np.int32)[rng.permutation(n)]
        held = old_ids[perm]                            # the old id of the marker in new slot j
        edge = np.isin(new_ids, (0, 1023))
        if (perm != np.arange(n)).all() and not np.isin(held[edge], (0, 1023)).any():
            break
    write_map(prm, orc_prm, new_ids, pos[perm], rot[perm])
    rename = {int(o): int(nw) for o, nw in zip(held, new_ids)}
    rename[-1] = -1

    def conv(a):
        a = np.asarray(a)
        assert np.isin(a, list(rename)).all(), "a measurement id outside the map cannot be relabelled"
        return np.vectorize(rename.get, otypes=[np.int32])(a).reshape(a.shape)
    return [conv(a) for a in ids] if isinstance(ids, (list, tuple)) else conv(ids)


def params(dialect):
    """the dialect's default parameters with the full map"""
    prm = capi.default_params(dialect)
    full_map(prm, None, SIZE)
    return prm


def oracle_engine(scene, batch=None, cov_form=oc.SIMPLE, prm=None):
    """the oracle with the scene's map (prm: another product parameter block's, e.g. the twin's)"""
    from replay_ref import OracleEngine
    eng = OracleEngine(batch or scene.B, scene.dialect, scene.nstate, cov_form=cov_form)
    write_map(capi.FbusParams.from_buffer_copy(prm or scene.prm), eng.orc.prm, *read_map(prm or scene.prm))
    return eng


# ---- scenes -------------------------------------------------------------------------------------------------------------------------------
MDRAW = 16                                   # every scene is drawn with 16 slots per filter and cut to M
PIXEL_SEED = {0: 42, 1: 41}                  # of util.pixel_scene, per dialect: chosen so that test_marker_map_cpu.py's coverage holds
TWIN_SEED = 12                               # of relabel(): likewise
_CACHE = {}


def _promote(ids, *arrays):
    """Reorders the slots of every filter so that the scenes cut to a small M still reach the edge slots: filter b moves the marker of
    one edge slot (b % 8 == 7: none) to its front if it sees it.  Filter 128 (b % 8 == 0) asks for slot 31, else the next slot down to
    26: the last, partly empty round of every copy.  In place."""
    want = ((31, 30, 29, 28, 27, 26), (12,), (15,), (16,), (25,), (26,), (0,), ())
    for b in range(len(ids)):
        for w in want[b % 8]:
            hit = np.nonzero(ids[b] == IDS[w])[0]
            if len(hit):
                j = int(hit[0])
                for a in (ids,) + arrays:
                    a[b, [0, j]] = a[b, [j, 0]]
                break


def _absent(ids, M):
    """scenes with M >= 3: every eighth filter (b % 8 == 7, never filter 128) loses one slot, walking through the M positions"""
    if M >= 3:
        for b in range(7, len(ids), 8):
            ids[b, (b // 8) % M] = -1


def _state(Bn, prm, nstate):
    nom, rot, P, prev = synth.initial_state(0, Bn, list(prm.p0_diag), nstate, mixed_cov=True)
    return nom, rot, P, prev


def pose_scene(Bn=B, M=4, dialect=0, nstate=18, frames=1):
    """Pose rows (synth.marker_frame) of `frames` camera frames on the full map, fp32-representable: namespace with prm, state = (nominal,
    rot, P, prev), ids (F, B, M), pos (F, B, M, 3), quat (F, B, M, 4) and 4 IMU samples.  prev: a marker of the filter's own frame 0 on
    three filters of four, id 0 on the fourth."""
    key = ("pose", Bn, M, dialect, nstate, frames)
    if key in _CACHE:
        return _CACHE[key]
    prm = params(dialect)
    nom, rot, P, _ = _state(Bn, prm, nstate)
    nom, rot, P = r32(nom), r32(rot), r32(P)
    rng = np.random.default_rng(1000 + 10 * dialect + nstate)
    ids, pos, quat = [], [], []
    for f in range(frames):
        i, p, q = synth.marker_frame(0, Bn, f, MDRAW, nom, prm)
        i, p, q = i.copy(), p + rng.normal(0, 0.02, p.shape), q.copy()       # innovations of a few cm
        _promote(i, p, q)
        i, p, q = i[:, :M].copy(), p[:, :M], q[:, :M]
        _absent(i, M)
        ids.append(i); pos.append(p); quat.append(q)
    ids, pos, quat = np.stack(ids), r32(np.stack(pos)), r32(np.stack(quat))
    pick = rng.integers(0, M, Bn)
    prev = np.where(np.arange(Bn) % 4 == 3, 0, np.maximum(ids[0, np.arange(Bn), pick], 0)).astype(np.int32)
    acc, gyr = synth.imu_samples(0, Bn, 0, 4, nom)
    s = types.SimpleNamespace(kind="pose", B=Bn, M=M, dialect=dialect, nstate=nstate, prm=prm, state=(nom, rot, P, prev),
                              ids=ids, pos=pos, quat=quat, acc=r32(acc), gyr=r32(gyr), dt=r32(np.full(4, 0.005)))
    _CACHE[key] = frozen(s)
    return s


def _corners_in_camera(prm, nom_b, slot):
    """the four corners of map slot `slot` in the left camera frame of the filter state nom_b (the forward model of util.pixel_scene)"""
    R_IL, P_IL, _ = synth.camera_constants(prm)
    _, mpos, mquat = synth.marker_table(prm)
    c = np.array([[0, 0, 0], [0, SIZE, 0], [SIZE, SIZE, 0], [SIZE, 0, 0.0]])
    R0 = synth.q2R(nom_b[6:10])
    world = mpos[slot] + (synth.q2R(mquat[slot]) @ c.T).T
    return (R_IL @ (R0.T @ (world - nom_b[0:3] - R0 @ P_IL).T)).T


def _pixel_draw(Bn, dialect, nstate):
    """one draw of util.pixel_scene per (B, dialect, N): 16 slots per filter from 1.2 - 1.8 m, promoted; every M cuts it"""
    key = ("draw", Bn, dialect, nstate)
    if key not in _CACHE:
        prm = params(dialect)
        nom0, _, P, prev = _state(Bn, prm, nstate)
        truth, _, ids, left, right = pixel_scene(Bn, MDRAW, prm, SIZE, seed=PIXEL_SEED[dialect], noise=5e-4, nominal=nom0, depth=(1.2, 1.8))
        _promote(ids, left, right)
        rng = np.random.default_rng(PIXEL_SEED[dialect] + 1)
        nom = truth.copy()
        nom[:, 0:3] += rng.normal(0, 0.004, (Bn, 3))                          # innovations of a few mm / mrad
        dq = np.concatenate([np.ones((Bn, 1)), rng.normal(0, 0.002, (Bn, 3))], axis=1)
        nom[:, 6:10] = synth.qmul(nom[:, 6:10], dq)
        nom[:, 6:10] /= np.linalg.norm(nom[:, 6:10], axis=1, keepdims=True)
        nom = r32(nom)
        rot = r32(synth.q2R(nom[:, 6:10]).reshape(Bn, 9))
        c3 = np.zeros((Bn, MDRAW, 12))
        slot_of = {i: k for k, i in enumerate(IDS)}
        for b in range(Bn):
            for m in range(MDRAW):
                if ids[b, m] >= 0:
                    c3[b, m] = _corners_in_camera(prm, truth[b], slot_of[int(ids[b, m])]).ravel()
        c3 += rng.normal(0, 0.003, c3.shape)                                  # triangulated corners: the true ones + 3 mm
        acc, gyr = synth.imu_samples(0, Bn, 0, 4, nom)
        _CACHE[key] = frozen((prm, (nom, rot, r32(P), prev), ids, r32(left), r32(right), r32(c3), r32(acc), r32(gyr)))
    return _CACHE[key]


def meas_scene(Bn=B, M=4, dialect=0, nstate=18):
    """Pixel rows (left, right: (B, M, 8)) and corner rows (c3: (B, M, 12), the corners themselves; or left / right triangulated) of
    ONE camera frame on the full map, fp32-representable.  prev as in pose_scene."""
    key = ("meas", Bn, M, dialect, nstate)
    if key in _CACHE:
        return _CACHE[key]
    prm, (nom, rot, P, prev), ids, left, right, c3, acc, gyr = _pixel_draw(Bn, dialect, nstate)
    ids = ids[:, :M].copy()
    _absent(ids, M)
    rng = np.random.default_rng(2000 + M)
    pick = rng.integers(0, M, Bn)
    prev = np.where(np.arange(Bn) % 4 == 3, 0, np.maximum(ids[np.arange(Bn), pick], 0)).astype(np.int32)
    s = types.SimpleNamespace(kind="meas", B=Bn, M=M, dialect=dialect, nstate=nstate, prm=prm, state=(nom, rot, P, prev),
                              ids=ids, left=np.ascontiguousarray(left[:, :M]), right=np.ascontiguousarray(right[:, :M]),
                              c3=np.ascontiguousarray(c3[:, :M]), acc=acc, gyr=gyr, dt=r32(np.full(4, 0.005)))
    _CACHE[key] = frozen(s)
    return s


def twin_of(scene, seed=TWIN_SEED):
    """the scene on the relabelled map: the same arrays, other ids and another parameter block"""
    key = ("twin", id(scene), seed)
    if key not in _CACHE:
        t = types.SimpleNamespace(**vars(scene))
        t.prm = capi.FbusParams.from_buffer_copy(scene.prm)
        prev = scene.state[3]
        t.ids, prev = relabel(t.prm, None, [scene.ids, prev], seed)
        t.rename = lambda a: relabel(capi.FbusParams.from_buffer_copy(scene.prm), None, a, seed)     # ids of the scene -> the twin's
        t.state = scene.state[:3] + (prev,)
        _CACHE[key] = (frozen(t), scene)                # (keeps `scene` alive: id() stays unique)
    return _CACHE[key][0]


def triangulated(scene):
    """the oracle's triangulation of the scene's image points: (B, M, 4, 3), what its corner-row update takes for the refractive geometry"""
    key = ("tri", id(scene))
    if key not in _CACHE:
        vp = oc.vision_params()
        out = np.zeros((scene.B, scene.M, 4, 3))
        for b in range(scene.B):
            for m in range(scene.M):
                if scene.ids[b, m] >= 0:
                    out[b, m] = oc.refraction_triangulate(vp, scene.left[b, m], scene.right[b, m])
        _CACHE[key] = (frozen(out), scene)
    return _CACHE[key][0]


# ---- the oracle's side of one update ------------------------------------------------------------------------------------------------------
def oracle_update(scene, what, mode=capi.MODE_STACKED, cov_form=oc.SIMPLE, state=None, frame=0, analytic=True, prm=None):
    """One update of the fp64 oracle from scene.state (or `state`): what = "pose" | "left" | "stereo" | "c3d" | "tri".
    Returns (state, applied)."""
    eng = oracle_engine(scene, cov_form=cov_form, prm=prm)
    eng.set_state(*(state or scene.state))
    o = eng.orc
    if what == "pose":
        ok = o.correct(eng.nominal, eng.rot, eng.P, eng.prev, scene.ids[frame], scene.pos[frame], scene.quat[frame], mode)
    elif what in ("left", "stereo"):
        fn = o.correct_pixels
        ok = fn(eng.nominal, eng.rot, eng.P, eng.prev, scene.ids, scene.left, scene.right if what == "stereo" else None, SIZE,
                scene.prm.r_pix, analytic=analytic)
    else:
        c = scene.c3.reshape(scene.B, scene.M, 4, 3) if what == "c3d" else triangulated(scene)
        ok = o.correct_corners(eng.nominal, eng.rot, eng.P, eng.prev, scene.ids, c, SIZE, mode)
    return eng.get_state(), ok


# ---- what the scenes must cover (asserted by tests/test_marker_map_cpu.py on every scene the GPU module uses) ---------------------------------
POSE_M = (1, 3, 5, 6, 7, 13, 16)
PIXEL_M = (1, 2, 3, 5, 7, 16)
CORNER_M = (1, 3, 5, 7)
PAD = ((3, 8), (5, 8), (7, 8), (13, 16))


def coverage(ids2d, prm=None):
    """of one frame's ids (B, M): filters folding each map slot, filters folding each id, the slots of the last filter"""
    table = list(IDS) if prm is None else [int(x) for x in read_map(prm)[0]]
    per_slot = np.array([(ids2d == i).any(axis=1).sum() for i in table])
    per_id = {i: int((ids2d == i).any(axis=1).sum()) for i in EDGE_IDS}
    last = [table.index(int(i)) for i in ids2d[-1] if i >= 0]
    return per_slot, per_id, last
