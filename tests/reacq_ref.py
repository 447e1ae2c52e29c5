"""Re-acquisition: one measurement update against a prior that has GROWN by orders of magnitude (a vehicle that lost sight of the markers and
gets a fix again), for tests/test_reacquisition_cpu.py and tests/test_reacquisition_gpu.py only -- never imported by the product package.

What is here:
  grown          the prior D P D with the sigmas of p and v scaled by s, the nominal state untouched
  meas_err       the relative error of the posterior ALONG THE MEASURED ROWS, max |H (P_got - P_ref) H'| / max |H P_ref H'|: the figure
                 util.cov_rel_err_blockwise cannot see for an update that is not of full rank (it scales every element by
                 sqrt(P_ii P_jj), and a one-row update leaves the block's diagonal large)
  record_floor   the same figures for the fp64 posterior rounded once to fp32: what no filter with an fp32 record can beat
  *_rows         the row matrices H of each kind, from the restatements that exist (depth_ref, velocity_ref, ekf_oracle_np._rows,
                 central differences of support.predicted_rows as tests/screen_ref.py takes them)
  seq32          the stacked update as DESIGN 4.2 and the comment block "Stacked mode: the information-compressed joint update" of
                 csrc/ekf_device.hpp define it -- Lam = sum h_J h_J' / r, Lam = L D L', six sequential scalar updates -- with every product
                 and every sum rounded to float32: what fp32 arithmetic of this algorithm achieves, written from those formulas and
                 not from the kernels
  ref_*          the fp64 references of each kind on get_state() arrays, in the literal form (I - K H) P or in Joseph's form"""
import types

import numpy as np

import depth_ref
import ekf_oracle_np as E
import oracle_capi as oc
import velocity_ref as V
from fbus_ekf import capi, synth
from sensor_families import Depth, Velocity
from support import B_IND, J, SIZE, aa2q, imu_of, perturbed_setup, pose_setup, predicted_rows, r32, state_batch
from util import cov_rel_err, cov_rel_err_blockwise

LADDER = (1, 10, 100)                                # prior sigma of p and v, times: at 1000 the rounded reference itself is indefinite


# ---- the prior ------------------------------------------------------------------------------------------------------------------------------
def grown(state, s):
    """get_state() arrays (nominal, rot, P, prev) -> the same with P <- D P D, D = diag(s on the error states of p and v (0..5), 1 on theta,
    the biases and g).  Formed in double and rounded to fp32 where the record is fp32; the nominal state, the carried rotation and prev
    are the ones given, so the kernel and the reference linearise at the same point."""
    nom, rot, P, prev = state
    d = np.ones(np.shape(P)[-1])
    d[0:6] = float(s)
    Pg = np.asarray(P, np.float64) * d[:, None] * d[None, :]
    Pg = (Pg + np.swapaxes(Pg, 1, 2)) / 2
    return nom, rot, Pg.astype(np.asarray(P).dtype), prev


# ---- the metric -----------------------------------------------------------------------------------------------------------------------------
def _rows_of(H, b):
    """H: one (m, N) matrix for every filter, or a sequence of B matrices (their row counts may differ)"""
    return np.asarray(H, np.float64) if isinstance(H, np.ndarray) and H.ndim == 2 else np.asarray(H[b], np.float64)


def meas_err_each(P_got, P_ref, H):
    P_got, P_ref = np.asarray(P_got, np.float64), np.asarray(P_ref, np.float64)
    out = np.zeros(len(P_ref))
    for b in range(len(P_ref)):
        Hb = _rows_of(H, b)
        out[b] = np.abs(Hb @ (P_got[b] - P_ref[b]) @ Hb.T).max() / np.abs(Hb @ P_ref[b] @ Hb.T).max()
    return out


def meas_err(P_got, P_ref, H):
    """max over the filters of max |H (P_got - P_ref) H'| / max |H P_ref H'|, H the m x N row matrix in fp64"""
    return float(meas_err_each(P_got, P_ref, H).max())


def record_floor(P_ref, H):
    """the figures of P_ref rounded once to fp32 against P_ref itself; "cov_block" and "cov" as util.assert_window_parity(floor=...) reads
    them, "meas" for meas_err"""
    P_ref = np.asarray(P_ref, np.float64)
    P32 = P_ref.astype(np.float32)
    return {"meas": meas_err(P32, P_ref, H), "cov_block": cov_rel_err_blockwise(P32, P_ref), "cov": cov_rel_err(P32, P_ref)}


def min_eig(P):
    """the smallest eigenvalue of every filter's P, in fp64"""
    return np.linalg.eigvalsh(np.asarray(P, np.float64)).min(axis=1)


# ---- row matrices ---------------------------------------------------------------------------------------------------------------------------
def depth_rows(state, n, axis, lever):
    a, lv = depth_ref.unit(axis), depth_ref.lever_of(lever)
    return [depth_ref.H_row(s, n, a, lv) for s in V.states_of(state, n)]


def velocity_rows(state, n, mount, lever, gyro):
    C, lv = V.mount_of(mount), V.lever_of(lever)
    return [V.H_rows(s, n, C, lv, None if gyro is None else gyro[b]) for b, s in enumerate(V.states_of(state, n))]


def folded_slots(s, prm, ids, pos, mode):
    """the slots of one filter that ekf_oracle_np.correct folds: all the ids of the map (stacked), or the nearest marker with the C++
    dialect's hysteresis on prev_id (nearest)"""
    ids = [int(i) for i in ids]
    if mode == E.STACKED:
        return [i for i, mid in enumerate(ids) if mid >= 0 and mid in prm.markers]
    mi, md, pi_, pd = -1, 10.0, -1, 0.0
    for i, mid in enumerate(ids):
        if mid < 0:
            continue
        d = np.linalg.norm(pos[i])
        if d < md:
            md, mi = d, i
        if prm.dialect == E.CPP and mid == s.prev_id:
            pd, pi_ = d, i
    if mi < 0:
        return []
    if prm.dialect == E.CPP and abs(pd - md) < prm.switch_thres and pd != 0:
        mi = pi_
    return [mi] if ids[mi] in prm.markers else []


def pose_rows(state, n, dialect, ids, pos, quat, mode):
    """per filter: the 7 rows (ekf_oracle_np._rows) of every folded slot, and their noise variances -> (list of H, list of r)"""
    prm = E.Params(dialect, n)
    Hs, rs = [], []
    for b, s in enumerate(V.states_of(state, n)):
        sel = folded_slots(s, prm, ids[b], np.asarray(pos[b], np.float64), mode)
        Hs.append(np.vstack([E._rows(s, prm, int(ids[b][i]), np.asarray(pos[b][i], np.float64), np.asarray(quat[b][i], np.float64))[0]
                             for i in sel]))
        rs.append(np.tile([prm.r_pos] * 3 + [prm.r_quat] * 4, len(sel)))
    return Hs, rs


def image_rows(state, n, prm, ids, kind, vp=None, eps=1e-6):
    """per filter: the rows in view of the pixel ("left" | "stereo") or corner ("corners") update, by central differences of the oracle's
    forward model (support.predicted_rows; the injection p += dp, q <- q (x) aa2q(dtheta)), as tests/screen_ref.py takes them; slots
    whose id is -1 or not in the map have no rows"""
    vp = vp if vp is not None else oc.vision_params()
    nom = np.asarray(state[0], np.float64)
    out = []
    for b in range(len(nom)):
        h0, vis = predicted_rows(nom[b], ids[b], prm, vp, kind)
        H = np.zeros((len(h0), n))
        for j in range(6):
            col = []
            for sg in (1.0, -1.0):
                d = np.zeros(6)
                d[j] = sg * eps
                x = nom[b].copy()
                x[0:3] += d[0:3]
                x[6:10] = synth.qmul(nom[b, 6:10][None], aa2q(d[3:6])[None])[0]
                col.append(predicted_rows(x, ids[b], prm, vp, kind)[0])
            H[:, J[j]] = (col[0] - col[1]) / (2 * eps)
        out.append(H[vis])
    return out


# ---- the stacked update in float32 ------------------------------------------------------------------------------------------------------------
def seq32(P, rows, r, f=np.float32):
    """P (N, N), rows (m, N) with their non-zeros in the columns J = (p, theta), r the noise variance of every row (a scalar or (m,)) ->
    the posterior in float32, every product and every sum rounded to float32:
        Lam = sum h_J h_J' / r  (6 x 6)      Lam = L D L'  (L unit lower triangular, no pivoting; a pivot that is not > 0 is a direction
        without information: a no-op)        for a = 0..5, with the row l = column a of L and the information d = D_a:
        u = P(:, J) l      P <- P - u u' d / (1 + d l'u_J)        (the scalar update with noise 1 / d; nothing divides by d)
    f = np.float64: the same steps in double, which the CPU suite holds to the dense reference to show that the algebra is right"""
    P = np.array(P, f)
    N = P.shape[0]
    rows = np.asarray(rows, np.float64)
    assert not rows[:, [c for c in range(N) if c not in J]].any(), "the rows have their non-zeros in J"
    h = rows[:, J].astype(f)
    w = (f(1) / np.broadcast_to(np.asarray(r, np.float64), (len(h),)).astype(f)).astype(f)
    Lam = np.zeros((6, 6), f)
    for k in range(len(h)):
        wh = (h[k] * w[k]).astype(f)
        Lam = (Lam + (wh[:, None] * h[k][None, :]).astype(f)).astype(f)
    L, D = np.eye(6, dtype=f), np.zeros(6, f)
    for a in range(6):
        d = Lam[a, a]
        D[a] = d
        if not d > 0:
            continue
        for i in range(a + 1, 6):
            L[i, a] = f(Lam[i, a] / d)
        for i in range(a + 1, 6):
            for j in range(a + 1, i + 1):
                Lam[i, j] = Lam[j, i] = f(Lam[i, j] - f(f(L[i, a] * d) * L[j, a]))
    for a in range(6):
        if not D[a] > 0:
            continue
        l = L[:, a]
        u = np.zeros(N, f)
        for k in range(a, 6):
            u = (u + (P[:, J[k]] * l[k]).astype(f)).astype(f)
        hph = f(0)
        for k in range(a, 6):
            hph = f(hph + f(l[k] * u[J[k]]))
        g = f(D[a] / f(f(1) + f(D[a] * hph)))
        T = ((u * g).astype(f)[:, None] * u[None, :]).astype(f)
        T = np.tril(T) + np.tril(T, -1).T                 # one rounding history for (i, j) and (j, i)
        P = (P - T).astype(f)
    return P


def seq32_batch(P, Hs, rs, f=np.float32):
    """seq32 on every filter: P (B, N, N), Hs a sequence of row matrices, rs one scalar, one vector for all, or a list of vectors"""
    return np.array([seq32(P[b], Hs[b], rs[b] if isinstance(rs, list) else rs, f) for b in range(len(P))])


# ---- references -----------------------------------------------------------------------------------------------------------------------------
def ref_depth(state, n, z, var, axis, offset, lever, joseph=False):
    ss = V.states_of(state, n)
    app = [depth_ref.correct_depth(s, n, float(z[b]), float(var), axis, offset, lever, joseph=joseph)[0] for b, s in enumerate(ss)]
    return V.arrays_of(ss), np.array(app)


def ref_velocity(state, n, z, var, gyro, mount, lever, joseph=False):
    ss = V.states_of(state, n)
    app = [V.correct_velocity(s, n, z[b], var, None if gyro is None else gyro[b], mount, lever, joseph=joseph)[0]
           for b, s in enumerate(ss)]
    return V.arrays_of(ss), np.array(app)


def _arrays(state):
    nom, rot, P = (np.array(x, np.float64, order="C") for x in state[:3])
    return nom, rot, P, np.array(state[3], np.int32)


def ref_pose(state, n, dialect, ids, pos, quat, mode, joseph=False):
    nom, rot, P, prev = _arrays(state)
    ok = oc.Oracle(dialect, n, oc.JOSEPH if joseph else oc.SIMPLE).correct(nom, rot, P, prev, ids, pos, quat, mode)
    return (nom, rot, P, prev), ok != 0


def ref_image(state, n, dialect, kind, ids, left, right, r_pix, joseph=False):
    """kind "left" | "stereo": the oracle's pixel rows with the closed-form d pi / d X; "corners": its corner rows, stacked"""
    nom, rot, P, prev = _arrays(state)
    orc = oc.Oracle(dialect, n, oc.JOSEPH if joseph else oc.SIMPLE)
    if kind == "corners":
        ok = orc.correct_corners(nom, rot, P, prev, ids, np.asarray(left, np.float64).reshape(len(nom), -1, 4, 3), SIZE, oc.STACKED)
    else:
        ok = orc.correct_pixels(nom, rot, P, prev, ids, left, right if kind == "stereo" else None, SIZE, r_pix, analytic=True)
    return (nom, rot, P, prev), ok != 0


# ---- the cells: inputs, readings, reference and rows of each kind ------------------------------------------------------------------------------
DEPTH = dict(axis=Depth.AXIS, offset=Depth.OFFSET, lever=Depth.LEVER, var=Depth.SENSOR_VAR)          # the sensors of tests/sensor_families.py
VELOCITY = dict(mount=Velocity.MOUNT, lever=Velocity.LEVER, var=Velocity.VAR)
KINDS = ("depth", "velocity", "pose_nearest", "pose_stacked", "left", "stereo", "corners")


def as_record(state, dtype):
    """the arrays as a handle with fp32 / fp64 records returns them"""
    t = np.float32 if dtype == 32 else np.float64
    return tuple(np.asarray(x).astype(t) for x in state[:3]) + (np.asarray(state[3], np.int32),)


def setup(kind, dtype, n, joseph=False, B=B_IND):
    """the parameters, the state and the inputs of one cell, built as the kind's own suite builds them: support.state_batch (depth,
    velocity: the suites run three predicts on it, c.acc / c.gyr are their samples and c.gyr[3] the rate sample of the velocity reading),
    support.pose_setup with the C++ dialect's seven live rows per marker, support.perturbed_setup (in-view scenes, every filter its own) with M = 4"""
    c = types.SimpleNamespace(kind=kind, dtype=dtype, n=n, B=B, joseph=joseph)
    if kind in ("depth", "velocity"):
        c.dialect = 0
        c.prm, nom, rot, P, prev = state_batch(B, c.dialect, n)
        c.acc, c.gyr = imu_of(0, B, 0, 4, nom)
    elif kind in ("pose_nearest", "pose_stacked"):
        c.dialect, c.mode = 1, (capi.MODE_NEAREST if kind == "pose_nearest" else capi.MODE_STACKED)
        c.prm, nom, rot, P, prev, c.ids, c.a, c.b = pose_setup(B, dtype, n, c.dialect, joseph)
    else:
        c.dialect = 0
        c.prm, nom, rot, P, prev, c.ids, c.a, c.b = perturbed_setup(B, dtype, n, c.dialect, kind, n=B)
    c.state = (nom, rot, P, prev)
    return c


def measure(c, state):
    """depth, velocity: the reading z = h(state) + noise of the sensor's size, representable in the record type (the suites' readings())"""
    rnd = r32 if c.dtype == 32 else (lambda a: np.asarray(a, np.float64))
    nom, rot = np.asarray(state[0], np.float64), np.asarray(state[1], np.float64).reshape(-1, 3, 3)
    rng = np.random.default_rng(5)
    if c.kind == "depth":
        hx = (nom[:, 0:3] + rot @ DEPTH["lever"]) @ depth_ref.unit(DEPTH["axis"]) + DEPTH["offset"]
        c.z = rnd(hx + rng.normal(0, 0.01, len(nom)))
    elif c.kind == "velocity":
        c.w = c.gyr[3]
        y = np.einsum("bji,bj->bi", rot, nom[:, 3:6]) + np.cross(c.w - nom[:, 13:16], VELOCITY["lever"])
        c.z = rnd(y @ VELOCITY["mount"].T + rng.normal(0, 1, (len(nom), 3)) * np.sqrt(VELOCITY["var"]))
    return c


def reference(c, state, joseph):
    """the fp64 restatement of the cell's update on `state` -> ((nominal, rot, P, prev), applied)"""
    if c.kind == "depth":
        return ref_depth(state, c.n, c.z, DEPTH["var"], DEPTH["axis"], DEPTH["offset"], DEPTH["lever"], joseph)
    if c.kind == "velocity":
        return ref_velocity(state, c.n, c.z, VELOCITY["var"], c.w, VELOCITY["mount"], VELOCITY["lever"], joseph)
    if c.kind in ("pose_nearest", "pose_stacked"):
        return ref_pose(state, c.n, c.dialect, c.ids, c.a, c.b, c.mode, joseph)
    return ref_image(state, c.n, c.dialect, c.kind, c.ids, c.a, c.b, c.prm.r_pix, joseph)


def rows(c, state):
    """(per-filter row matrices, their noise variances: a scalar, one vector, or a list of vectors)"""
    if c.kind == "depth":
        return depth_rows(state, c.n, DEPTH["axis"], DEPTH["lever"]), DEPTH["var"]
    if c.kind == "velocity":
        return velocity_rows(state, c.n, VELOCITY["mount"], VELOCITY["lever"], c.w), VELOCITY["var"]
    if c.kind in ("pose_nearest", "pose_stacked"):
        return pose_rows(state, c.n, c.dialect, c.ids, c.a, c.b, E.NEAREST if c.kind == "pose_nearest" else E.STACKED)
    return image_rows(state, c.n, c.prm, c.ids, c.kind), (c.prm.r_pos if c.kind == "corners" else c.prm.r_pix)
