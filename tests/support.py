"""What more than one test module needs: rounding, constants, the environment-knob context manager, state and input builders, handles and
calls, bit-equality of states and of named outputs, the builders of the independence variants.  A plain library: no tests and no pytest
marks, importable without a GPU.  tests/route_cells.py (and through it tools/route_matrix.py) builds its cells from it.

Every builder here feeds bit-for-bit comparisons downstream: seeds, the order of the random draws, the point where values are rounded,
dtypes and contiguity are part of each function's contract.  Where two helpers differ in one of these they are two functions, side by
side, and their docstrings say how they differ."""
import contextlib
import math
import os
import types

import numpy as np
import torch

import oracle_capi as oc
from fbus_ekf import BatchedFilter, capi, noise, synth
from util import pixel_scene

SIZE = 0.28                                  # marker edge [m] of the pixel / corner scenes (tests/marker_maps.py has its own scene and size)
DT = np.array([np.float64(np.float32(0.005))])     # one fp32-representable IMU period, as the (1,) fp64 array predict() takes
J = [0, 1, 2, 6, 7, 8]                       # error-state columns of position and attitude


def r32(a):
    """round to fp32-representable values, returned as float64: the GPU (fp32) and the oracle (fp64) see IDENTICAL inputs"""
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


@contextlib.contextmanager
def env(**kw):
    """environment knobs are read ONCE, at fbus_ekf_create: set them around the construction of a handle"""
    before = {k: os.environ.get(k) for k in kw}
    os.environ.update({k: str(v) for k, v in kw.items()})
    try:
        yield
    finally:
        for k, v in before.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def frozen(x):
    """x with every array in it (tuples, lists and namespaces are walked) refusing writes: what a cache hands out"""
    if isinstance(x, np.ndarray):
        x.setflags(write=False)
    elif isinstance(x, (tuple, list)):
        for y in x:
            frozen(y)
    elif isinstance(x, types.SimpleNamespace):
        for y in vars(x).values():
            frozen(y)
    return x


# ---- the fp32-record floor of a free-running window (util.assert_window_parity) ------------------------------------------------------
def round_records(nominal, rot, P):
    """the record arrays rounded to fp32 IN PLACE: what an exact-arithmetic filter with fp32 records keeps of a step's result"""
    nominal[...] = r32(nominal); rot[...] = r32(rot); P[...] = r32(P)


def fp32_record_floor(run):
    """run(fp32_records) -> (nominal, rot, P, ...): the fp64 reference of a window, with fp32_records=True the same arithmetic with the
    record rounded to fp32 after every step (round_records).  -> (the fp64 run, util.parity_errors of the rounded run against it): the
    `floor` of util.assert_window_parity"""
    from util import parity_errors
    ref = run(False)
    return ref, parity_errors(run(True), ref)


# ---- bit-equality -------------------------------------------------------------------------------------------------------------------
def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(f"u{x.dtype.itemsize}")


def same_rows(a, b, rows=None, rows_b=None):
    """dicts name -> array with the filters along axis 0: a[name][rows] and b[name][rows_b] hold the same BITS for every name of a (NaN
    equals the same NaN, 0.0 does not equal -0.0).  rows / rows_b: index arrays, None = all.  Prints which names differ, in how many of
    the filters and in which (numbered as in a)."""
    ra, rb = (slice(None) if r is None else np.asarray(r) for r in (rows, rows_b))
    ok = True
    for name, x in a.items():
        x, y = np.asarray(x)[ra], np.asarray(b[name])[rb]
        if x.shape != y.shape or x.dtype != y.dtype:
            print(f"differs: {name} is {x.dtype} {x.shape} and {y.dtype} {y.shape}")
            ok = False
            continue
        d = (_bits(x) != _bits(y)).reshape(len(x), -1)
        if d.any():
            ok = False
            with np.errstate(invalid="ignore"):
                diff = np.abs(x.astype(np.float64) - y.astype(np.float64)).reshape(len(x), -1)
            who = np.nonzero(d.any(axis=1))[0]
            who = who if rows is None else np.asarray(rows)[who]
            print(f"differs: {name} in {len(who)} filters {who[:12]}, columns {np.nonzero(d.any(axis=0))[0][:12]}, "
                  f"max |diff| {np.nanmax(diff):.3e}")
    return ok


def same_state(a, b, rows=None):
    """every array of a equals its partner in b bit for bit (on the filters `rows`): (nominal, rot, P, prev), with or without `applied` as
    a fifth.  Prints where they differ."""
    sel = slice(None) if rows is None else rows
    ok = all(np.array_equal(x[sel], y[sel]) for x, y in zip(a, b))
    if not ok:
        for name, x, y in zip(("nominal", "rot", "P", "prev", "applied"), a, b):
            x, y = np.asarray(x)[sel], np.asarray(y)[sel]
            if x.shape != y.shape:
                print(f"differs: {name} has shapes {x.shape} and {y.shape}")
                continue
            d = x.reshape(len(x), -1) != y.reshape(len(y), -1)
            if d.any():
                diff = np.abs(x.astype(np.float64) - y.astype(np.float64)).reshape(len(x), -1)
                print(f"differs: {name} in {int(d.any(axis=1).sum())} filters, columns {np.nonzero(d.any(axis=0))[0][:12]}, "
                      f"max |diff| {diff.max():.3e}")
    return ok


# ---- the same filters in other surroundings (tests/test_independence_*.py) ----------------------------------------------------------------
B_IND = 193                                  # three full 64-filter tiles and a tile of one filter; prime


def permutation(B=B_IND, power=5, shift=106):
    """pi: position j holds filter pi[j] = (j ** power + shift) mod B.  B prime and power coprime to B - 1: a bijection.  (An affine map
    k j + c will not do: with k != 1 it has a fixed point, with k = 1 it is a rotation, which keeps every filter beside its neighbour.)"""
    return np.array([(pow(j, power, B) + shift) % B for j in range(B)])


def ragged_cut(B=B_IND, at=101):
    """two shards whose border lies inside a tile: at = 101 is lane 37 of tile 1, and the second shard ends in a tile of (B - at) % 64"""
    return np.arange(0, at), np.arange(at, B)


POISON_FORMS = 5                             # a b c d e of poisoned_state / with_nan
ALONE = (0, 100, 192)                        # the filters that also run on handles of one filter: first, mid-tile, the tail tile's only one


def poison_set(B=B_IND):
    """(S, form): the filters to break -- id % 7 == 5, all of tile 1 (64 .. 127) except 100 (a whole wave but one lane) and B - 2 -- and
    the form of each, cycling through all of them in the order of S"""
    b = np.arange(B)
    S = b[(b % 7 == 5) | ((b >= 64) & (b < 128) & (b != 100)) | (b == B - 2)]
    return S, np.arange(len(S)) % POISON_FORMS


def poisoned_state(nom, rot, P, S, form):
    """copies of (nominal, rot, P) with the filters S broken, S[i] in the way form[i]: 0 (a) NaN in all three; 1 (b) position +Inf and the
    covariance diagonal 1e30; 2 (c) the covariance -P; 4 (e) zero quaternion and zero rotation; 3 (d) leaves the state alone (with_nan
    breaks its inputs)"""
    nom, rot, P = np.array(nom), np.array(rot), np.array(P)
    a, b, c, e = (S[form == k] for k in (0, 1, 2, 4))
    nom[a], rot[a], P[a] = np.nan, np.nan, np.nan
    nom[b, 0:3] = np.inf
    i = np.arange(P.shape[1])
    P[b[:, None], i, i] = 1e30
    P[c] = -P[c]
    nom[e, 6:10], rot[e] = 0.0, 0.0
    return nom, rot, P


def with_nan(x, where, axis):
    """a copy of x, NaN at the indices `where` of `axis`"""
    x = np.array(x)
    x[(slice(None),) * axis + (where,)] = np.nan
    return x


# ---- pose-row states and inputs, fp32-representable -----------------------------------------------------------------------------------
def params_of(dialect, cov_form=0):
    p = capi.default_params(dialect)
    p.cov_form = cov_form
    return p


def state_batch(B, dialect, n, mixed=True, seed_off=0):
    """the dialect's parameters and filters seed_off .. seed_off + B of synth.initial_state"""
    prm = params_of(dialect)
    nom, rot, P, prev = synth.initial_state(seed_off, seed_off + B, list(prm.p0_diag), n, mixed_cov=mixed)
    return prm, r32(nom), r32(rot), r32(P), prev


def imu_of(lo, hi, step, K, nom):
    """K samples from `step` on for filters lo .. hi, rounded always, without periods (imu(): filters 0 .. B, rounded for fp32 only)"""
    a, g = synth.imu_samples(lo, hi, step, K, nom)
    return r32(a), r32(g)


def markers_of(lo, hi, frame, M, nom, prm):
    """one frame of pose rows, rounded always (pose_setup rounds for fp32 records only)"""
    ids, pos, quat = synth.marker_frame(lo, hi, frame, M, nom, prm)
    return ids, r32(pos), r32(quat)


def state_of(B, dtype, nstate, dialect):
    """(parameters, state) of filters 0 .. B; rounded for fp32 records only (state_batch rounds always)"""
    prm = capi.default_params(dialect)
    nom, rot, P, prev = synth.initial_state(0, B, list(prm.p0_diag), nstate, mixed_cov=True)
    if dtype == 32:
        nom, rot, P = r32(nom), r32(rot), r32(P)
    return prm, (nom, rot, P, prev)


def imu(B, K, nom, dtype):
    """K samples and their periods; rounded for fp32 records only.  The period is 0.005 itself in fp64: not DT"""
    a, w = synth.imu_samples(0, B, 0, K, nom)
    dt = np.full(K, 0.005)
    if dtype == 32:
        a, w, dt = r32(a), r32(w), r32(dt)
    return a, w, dt


def pose_setup(B, dtype, nstate, dialect, joseph, M=4):
    """parameters, state and frame 0 of pose rows for filters 0 .. B in one tuple; rounded for fp32 records only"""
    prm = capi.default_params(dialect)
    if joseph:
        prm.cov_form = capi.COV_JOSEPH
    nom, rot, P, prev = synth.initial_state(0, B, list(prm.p0_diag), nstate, mixed_cov=True)
    ids, pos, quat = synth.marker_frame(0, B, 0, M, nom, prm)
    if dtype == 32:
        nom, rot, P, pos, quat = (r32(a) for a in (nom, rot, P, pos, quat))
    return prm, nom, rot, P, prev, ids, pos, quat


# ---- pixel, stereo and corner scenes -----------------------------------------------------------------------------------------------
TILT = np.array([0.03, -0.02, 1.0]) / np.linalg.norm([0.03, -0.02, 1.0])


def vp_tilted():
    vp = oc.vision_params()
    for i in range(3):
        vp.normal[i] = float(TILT[i])
    return vp


def aa2q(v):
    th = np.linalg.norm(v)
    if th == 0.0:
        return np.array([1.0, 0.0, 0.0, 0.0])
    return np.concatenate([[math.cos(th / 2)], math.sin(th / 2) * v / th])


def predicted_rows(nom, ids_b, prm, vp, kind):
    """predicted rows of one filter (marker slots in order, corners 0..3; pixels: left (+ right) per corner; corners: xyz) and
    the visibility of each row"""
    R_IL, P_IL, _ = synth.camera_constants(prm)
    mids, mpos, mquat = synth.marker_table(prm)
    c = np.array([[0, 0, 0], [0, SIZE, 0], [SIZE, SIZE, 0], [SIZE, 0, 0.0]])
    R0 = synth.q2R(nom[6:10])
    rows, vis = [], []
    for mid in ids_b:
        if mid < 0 or mid not in mids:
            continue
        k = list(mids).index(mid)
        world = mpos[k] + (synth.q2R(mquat[k]) @ c.T).T
        cam = (R_IL @ (R0.T @ (world - nom[0:3] - R0 @ P_IL).T)).T
        if kind == "corners":
            rows.append(cam.ravel()); vis += [True] * 12
            continue
        uvL, uvR, ok = oc.project_stereo(vp, cam, stereo=kind == "stereo")
        for q in range(4):
            rows.append(uvL[q]); vis += [ok[q]] * 2
            if kind == "stereo":
                rows.append(uvR[q]); vis += [ok[q]] * 2
    return np.concatenate(rows), np.array(vis, bool)


def measured_rows(ids_b, left_b, right_b, prm, kind):
    mids = list(synth.marker_table(prm)[0])
    y = []
    for m, mid in enumerate(ids_b):
        if mid < 0 or mid not in mids:
            continue
        if kind == "corners":
            y.append(left_b[m]); continue
        for q in range(4):
            y.append(left_b[m, 2 * q:2 * q + 2])
            if kind == "stereo":
                y.append(right_b[m, 2 * q:2 * q + 2])
    return np.concatenate(y)


_SCENES = {}


def truth_scene(n, M, seed, noise, tilted=False, prior_dialect=0):
    """(nominal of the initial state, P, prev, truth, ., ids, left, right) of util.pixel_scene for n filters, cached and read-only.
    tilted: the port normal TILT.  prior_dialect: the dialect whose p0_diag seeds P -- nothing else of the scene depends on a dialect"""
    key = (n, M, seed, noise, tilted, prior_dialect)
    if key not in _SCENES:
        prm = capi.default_params(0)
        prm.marker_size = SIZE
        if tilted:
            for i in range(3):
                prm.port_normal[i] = float(TILT[i])
        p0 = list(capi.default_params(prior_dialect).p0_diag)
        nom0, _, P, prev = synth.initial_state(0, n, p0, 18, mixed_cov=True)
        vision = {"vision": vp_tilted()} if tilted else {}
        _SCENES[key] = frozen((nom0, P, prev) + tuple(pixel_scene(n, M, prm, SIZE, seed=seed, noise=noise, nominal=nom0, **vision)))
    return _SCENES[key]


def perturbed_setup(B, dtype, nstate, dialect, kind, M=4, seed=3, n=256, tilted=False, prior_dialect=0):
    """B filters (an n-filter scene tiled), perturbed by a few mm / mrad from the truth: (prm, nominal, rot, P, prev, ids, left, right),
    fresh arrays.  kind: "left" | "stereo" (pixel rows) | "corners" (left = the triangulated corners).  The prior comes from
    prior_dialect's p0_diag whatever `dialect` is (tests/test_nis_gpu.py and its kin: 0; tests/test_pixels_gpu.py: the dialect itself)"""
    prm = capi.default_params(dialect)
    prm.marker_size = SIZE
    if tilted:
        for i in range(3):
            prm.port_normal[i] = float(TILT[i])
    nom0, P, prev, truth, _, ids, left, right = truth_scene(n, M, seed, 5e-4, tilted, prior_dialect)
    rep = (B + n - 1) // n
    tile = lambda a: np.concatenate([a] * rep)[:B]
    truth, P, prev, ids, left, right = map(tile, (truth, P, prev, ids, left, right))
    rng = np.random.default_rng(seed + 1)
    nom = truth.copy()
    nom[:, 0:3] += rng.normal(0, 0.004, (B, 3))
    nom[:, 6:10] = synth.qmul(nom[:, 6:10], np.concatenate([np.ones((B, 1)), rng.normal(0, 0.002, (B, 3))], axis=1))
    nom[:, 6:10] /= np.linalg.norm(nom[:, 6:10], axis=1, keepdims=True)
    P = P[:, :nstate, :nstate]
    if kind == "corners":                             # triangulated corners: the true ones + 3 mm
        left = np.zeros((B, M, 12))
        for b in range(n):
            h, _ = predicted_rows(truth[b], ids[b], prm, None, "corners")
            left[b, :len(h) // 12] = h.reshape(-1, 12)
        left = tile(left[:n]) + rng.normal(0, 0.003, left.shape)
    if dtype == 32:
        nom, P, left, right = r32(nom), r32(P), r32(left), r32(right)
    rot = synth.q2R(nom[:, 6:10]).reshape(B, 9)
    if dtype == 32:
        rot = r32(rot)
    return prm, nom, rot, P, prev, ids, left, right


# ---- handles and calls --------------------------------------------------------------------------------------------------------------
def to_device(a, dt=None):
    """a (None stays None, a tensor stays the tensor it is) on the device, cast to dt by numpy on the host first"""
    return a if a is None or torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()


def device_caster(torch, dtype):
    """a -> device tensor in the record type: integers as they are, everything else uploaded as fp64 and cast ON THE DEVICE (to_device
    casts on the host; no test compares the two, so they stay two)"""
    dev = torch.device("cuda:0")
    tt = torch.float32 if dtype == 32 else torch.float64
    return lambda a: (torch.from_numpy(np.ascontiguousarray(a)).to(dev) if np.asarray(a).dtype.kind in "iu"
                      else torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(dev).to(tt))


def make_filter(B, prm, dtype, nstate, state, roles=0):
    """a handle in `state` with the library's own team choice, or roles > 0: the correct kernels pinned to that many (set_team(0, roles))"""
    f = BatchedFilter(B, prm, device=0, dtype=dtype, nstate=nstate)
    f.set_state(*state)
    if roles:
        f.set_team(0, roles)
    return f


def update_call(f, kind, ids, left, right, nis=False, mode=capi.MODE_STACKED, skip=None, host=False):
    """one update through the device entry points (host=True: the host-pointer ones, numpy in and out); kind "pose": left = pos,
    right = quat"""
    npd = f.np_dtype
    conv = (lambda a, dt=None: None if a is None else np.ascontiguousarray(a, dt)) if host else to_device
    di, dl = conv(ids, np.int32), conv(left, npd)
    dr = conv(right, npd) if kind in ("stereo", "pose") else None
    ds = None if skip is None else conv(skip, np.uint8)
    if kind == "pose":
        out = (f.correct_nis if nis else f.correct)(di, dl, dr, mode, ds)
    elif kind == "corners":
        out = (f.correct_corners_nis if nis else f.correct_corners)(di, dl, None, capi.VIS_CORNERS3D, mode, ds)
    else:
        out = (f.correct_pixels_nis if nis else f.correct_pixels)(di, dl, dr, ds)
    f.sync()
    if nis:
        if host:
            return out[0].astype(np.float64), out[1]
        return out[0].cpu().numpy().astype(np.float64), out[1].cpu().numpy()
    return None


# ---- per-filter noise tables and their twins ----------------------------------------------------------------------------------------
G = 5
B_ODD = 4160 + 37                              # a partial last tile
FACT = np.array([0.1, 0.3, 1.0, 3.0, 10.0])


def rows_of(prm):
    """G rows, column c of row g = default x FACT[(g + 2c) % G]: every row differs from every other in every column"""
    base = noise.row_of(prm)
    return np.array([[base[c] * FACT[(g + 2 * c) % G] for c in range(7)] for g in range(G)])


def with_row(prm, row):
    p = capi.FbusParams.from_buffer_copy(prm)
    for i in range(4):
        p.q_diag[i] = float(row[i])
    p.r_pos, p.r_quat, p.r_pix = float(row[4]), float(row[5]), float(row[6])
    return p


def handle(B, prm, dtype, nstate, state, pin=True, policy_batch=0):
    """a handle in `state`, by default pinned to the one-wave forms of predict AND correct (make_filter pins correct alone, and only on
    request); policy_batch: the size class the routes are chosen for"""
    f = BatchedFilter(B, prm, device=0, dtype=dtype, nstate=nstate)
    f.set_state(*state)
    if pin:
        f.set_team(1, 1)                       # the one-wave forms (what a tabled handle runs)
    if policy_batch:
        f.set_policy_batch(policy_batch)
    return f


def run_twins(B, prm, dtype, nstate, state, step, pin=True, policy_batch=0):
    """step(handle) on a tabled handle and on G twins; returns the tabled handle's outputs and, per filter, the twin's"""
    rows = rows_of(prm)
    g = np.arange(B) % G
    with handle(B, prm, dtype, nstate, state, pin, policy_batch) as f:
        f.set_noise(rows[g])
        out = step(f)
        st = f.get_state()
        app = f.applied()
    ref_out, ref_st, ref_app = None, None, None
    for k in range(G):
        with handle(B, with_row(prm, rows[k]), dtype, nstate, state, pin, policy_batch) as t:
            o = step(t)
            s = t.get_state()
            a = t.applied()
        sel = g == k
        if ref_st is None:
            ref_st = [np.array(x) for x in s]
            ref_app = np.array(a)
            ref_out = None if o is None else [np.array(x) for x in o]
        for x, y in zip(ref_st, s):
            x[sel] = y[sel]
        ref_app[sel] = a[sel]
        if o is not None:
            for x, y in zip(ref_out, o):
                x[sel] = y[sel]
    return (st, app, out), (ref_st, ref_app, ref_out)


def assert_twin(got, ref, near_nominal=False):
    (st, app, out), (rst, rapp, rout) = got, ref
    if near_nominal:                            # fp64 C++-dialect stacked pose through the NIS kernel (include/fbus_ekf.h)
        np.testing.assert_allclose(st[0], rst[0], rtol=0, atol=2e-15)
        assert all(np.array_equal(x, y) for x, y in zip(st[1:], rst[1:]))
    else:
        assert same_state(st, rst)
    assert np.array_equal(app, rapp)
    if out is not None:
        assert all(np.array_equal(x, y) for x, y in zip(out, rout))
