"""fp64 numpy restatement of fbus_ekf_project_markers (include/fbus_ekf.h), for the tests only: written from the header's definition,
not from the device code.  X from the state arrays with the CARRIED rotation `rot` (not q2R(q)); the in-view rule in closed form, per
camera; uv from the oracle's forward projection (oracle_capi.project_stereo); H by central differences through the injection
(p + d_p, R Exp(d_theta)), as tests/screen_ref.py::image_slot does; S = H P_JJ H' + r I.  Never imported by the product package."""
import numpy as np

import oracle_capi as oc
from fbus_ekf import synth
from support import J, aa2q

FLIP = np.array([-1.0, -1.0, 1.0])           # left camera frame of the triangulation <-> refraction frame (vision.cpp:597-599)
LANES = (0, 63, 64, 127, 128, 129)


def subset(B):
    """the filters the reference is evaluated on: the rims of the tiles, the tail, and every 7th"""
    return sorted(set(k for k in LANES if k < B) | set(range(0, B, 7)))


def cameras_of(prm):
    """R_IL, P_IL, R_RL^-1, P_LR, the port normal, d_air + d_glass, klim"""
    R_IL, P_IL, _ = synth.camera_constants(prm)
    TL = np.array(list(prm.T_SC_left), float).reshape(4, 4)
    TR = np.array(list(prm.T_SC_right), float).reshape(4, 4)
    R_RL = TL[:3, :3] @ TR[:3, :3].T
    P_LR = TL[:3, 3] - R_RL @ TR[:3, 3]
    a1 = prm.n_air / prm.n_water
    return R_IL, P_IL, np.linalg.inv(R_RL), P_LR, np.array(list(prm.port_normal), float), prm.d_air + prm.d_glass, 0.81 * a1 * a1 / (1 - a1 * a1)


def corners_world(prm, k):
    """the four corners of map slot k in the world"""
    _, mpos, mquat = synth.marker_table(prm)
    s = prm.marker_size
    c = np.array([[0, 0, 0], [0, s, 0], [s, s, 0], [s, 0, 0.0]])
    return mpos[k] + (synth.q2R(mquat[k]) @ c.T).T


def corners_cam(p, R, prm, k):
    """the four corners of map slot k in the left camera frame (4, 3), as the oracle's projection takes them: R_IL (R'(c_w - p) - pil),
    pil = R'(R P_IL) taken literally"""
    R_IL, P_IL = cameras_of(prm)[:2]
    pil = R.T @ (R @ P_IL)
    return (R_IL @ ((R.T @ (corners_world(prm, k) - p).T).T - pil).T).T


def in_view(Xcam, prm, shift=None):
    """(..., 2) bool: left, right.  z_w = n.X - d_air - d_glass > 0 and |X - (n.X) n|^2 < klim z_w^2 in each camera's refraction frame;
    shift: a displacement (3,) in that camera's own frame (the stability probe of the rim tests)"""
    _, _, Rinv, P_LR, n, d, klim = cameras_of(prm)
    XL = np.asarray(Xcam, float) * FLIP
    XR = np.einsum("ij,...j->...i", Rinv, XL - P_LR)
    out = []
    for X in (XL, XR):
        X = X if shift is None else X + shift
        z = X @ n
        lat = X - z[..., None] * n
        zw = z - d
        out.append((zw > 0) & ((lat * lat).sum(-1) < klim * zw * zw))
    return np.stack(out, axis=-1)


def stable(Xcam, prm, move=0.005):
    """(...,) bool: the two flags of every point stay as they are when the point is moved by +-move along each camera axis"""
    ref = in_view(Xcam, prm)
    ok = np.ones(ref.shape[:-1], bool)
    for i in range(3):
        for s in (move, -move):
            d = np.zeros(3); d[i] = s
            ok &= (in_view(Xcam, prm, d) == ref).all(axis=-1)
    return ok


def depth_behind(Xcam, prm):
    """(..., 2): z_w of the point in the two cameras"""
    _, _, Rinv, P_LR, n, d, _ = cameras_of(prm)
    XL = np.asarray(Xcam, float) * FLIP
    XR = np.einsum("ij,...j->...i", Rinv, XL - P_LR)
    return np.stack([XL @ n - d, XR @ n - d], axis=-1)


def slot_of(prm, mid):
    mids = list(synth.marker_table(prm)[0])
    return mids.index(mid) if mid >= 0 and mid in mids else -1


def view_bits(nom, rot, ids, prm, cameras, skip=None):
    """view (B, M) uint8 of the header's rule 2 for every filter, in closed form"""
    Bn, M = ids.shape
    out = np.zeros((Bn, M), np.uint8)
    for b in range(Bn):
        if skip is not None and skip[b]:
            continue
        for m in range(M):
            k = slot_of(prm, int(ids[b, m]))
            if k < 0:
                continue
            f = in_view(corners_cam(nom[b, 0:3], rot[b].reshape(3, 3), prm, k), prm)
            for c in range(cameras):
                for q in range(4):
                    out[b, m] |= np.uint8(int(f[q, c]) << (4 * c + q))
    return out


def _uv(p, R, prm, vp, k, cameras):
    X = corners_cam(p, R, prm, k)
    uvL, uvR, _ = oc.project_stereo(vp, X, stereo=cameras == 2)
    return np.stack([uvL, uvR] if cameras == 2 else [uvL])          # (cameras, 4, 2)


def project(state, ids, prm, cameras, filters, vp=None, r_pix=None, cov=True, eps=1e-6):
    """-> left, right (B, M, 8), cov_left, cov_right (B, M, 4, 3), view (B, M) for the filters `filters` (rows of the others are zero).
    state: (nominal, rot, P) as the record holds them.  r_pix: scalar or (B,)"""
    nom, rot, P = (np.asarray(x, np.float64) for x in state[:3])
    vp = vp if vp is not None else oc.vision_params()
    Bn, M = ids.shape
    uv = np.zeros((2, Bn, M, 8))
    S = np.zeros((2, Bn, M, 4, 3))
    view = np.zeros((Bn, M), np.uint8)
    r = np.broadcast_to(np.asarray(prm.r_pix if r_pix is None else r_pix, float), (Bn,))
    for b in filters:
        p, R = nom[b, 0:3], rot[b].reshape(3, 3)
        PJJ = P[b][np.ix_(J, J)]
        for m in range(M):
            k = slot_of(prm, int(ids[b, m]))
            if k < 0:
                continue
            f = in_view(corners_cam(p, R, prm, k), prm)
            h0 = _uv(p, R, prm, vp, k, cameras)
            if cov:
                H = np.zeros((cameras, 4, 2, 6))
                for j in range(6):
                    col = []
                    for s in (1.0, -1.0):
                        d = np.zeros(6); d[j] = s * eps
                        col.append(_uv(p + d[0:3], R @ synth.q2R(aa2q(d[3:6])), prm, vp, k, cameras))
                    H[..., j] = (col[0] - col[1]) / (2 * eps)
            for c in range(cameras):
                for q in range(4):
                    if not f[q, c]:
                        continue
                    view[b, m] |= np.uint8(1 << (4 * c + q))
                    uv[c, b, m, 2 * q:2 * q + 2] = h0[c, q]
                    if cov:
                        Sq = H[c, q] @ PJJ @ H[c, q].T + r[b] * np.eye(2)
                        S[c, b, m, q] = (Sq[0, 0], Sq[0, 1], Sq[1, 1])
    return uv[0], uv[1], S[0], S[1], view


def cov_error(got, ref):
    """max |dS_ij| / sqrt(S_ii S_jj) over the projections that are in view in ref ((..., 3) = uu, uv, vv)"""
    on = ref[..., 0] > 0
    if not on.any():
        return 0.0
    g, r = got[on], ref[on]
    su, sv = np.sqrt(r[:, 0]), np.sqrt(r[:, 2])
    d = np.abs(g - r) / np.stack([su * su, su * sv, sv * sv], axis=1)
    return float(d.max())


def rim_scene(nom, rot, ids, prm):
    """For the rim tests: per filter one marker of the map that its frame does NOT list -- a stable partly visible one (some but not all
    of its 8 flags set, none of them changing under stable()'s move) where the filter has one, else one wholly behind the port of both
    cameras by more than 5 cm.  -> (pick (B,) int32, partly (B,) bool, n_unlisted, n_unstable)"""
    mids = synth.marker_table(prm)[0]
    Bn = len(nom)
    pick, partly = np.full(Bn, -1, np.int32), np.zeros(Bn, bool)
    n_unlisted = n_unstable = 0
    for b in range(Bn):
        p, R = nom[b, 0:3], rot[b].reshape(3, 3)
        behind = -1
        for k, mid in enumerate(mids):
            if mid in ids[b]:
                continue
            n_unlisted += 1
            X = corners_cam(p, R, prm, k)
            f, st = in_view(X, prm), stable(X, prm)
            if not st.all():
                n_unstable += 1
                continue
            if f.any() and not f.all() and not partly[b]:
                pick[b], partly[b] = mid, True
            if behind < 0 and (depth_behind(X, prm) < -0.05).all():
                behind = mid
        if not partly[b]:
            pick[b] = behind
    return pick, partly, n_unlisted, n_unstable
