"""fp64 numpy restatement of the per-marker screen (include/fbus_ekf.h, fbus_ekf_screen_markers), for the tests only: written from the
header's definition, not from the device code.  Per slot m of a filter: r' (H P H' + R)^-1 r over the rows the kind's stacked update
folds for a frame that holds slot m alone -- pixel and corner rows with H by central differences of the oracle's forward model
(support.predicted_rows, the injection of MeasureUpdate.m:91-98), pose rows with the oracle's own h, H, r (oracle_capi.Oracle.measurement)
-- then the decision nis <= thr[dof].  Never imported by the product package."""
import numpy as np

import oracle_capi as oc
from fbus_ekf import synth
from support import J, aa2q, measured_rows, predicted_rows

KIND_OF = {"pose": 0, "left": 1, "stereo": 1, "corners": 2}          # capi.SCREEN_*


def in_map(ids, prm):
    """which entries of ids are ids of the marker map"""
    return np.isin(np.asarray(ids), np.asarray(synth.marker_table(prm)[0])) & (np.asarray(ids) >= 0)


def alone(ids_b, m):
    """the ids of one filter with every slot but m absent"""
    out = np.full(len(ids_b), -1, np.int32)
    out[m] = ids_b[m]
    return out


def image_slot(nom, P, ids_b, left_b, right_b, prm, kind, m, vp=None, eps=1e-6, r_meas=None):
    """(nis, dof, sum r^2 / R) of slot m of one filter, kind "left" | "stereo" | "corners"; None for a slot that is not judged (its id
    is not in the map, or none of its rows is in view)"""
    if not in_map(ids_b[m:m + 1], prm)[0]:
        return None
    vp = vp if vp is not None else oc.vision_params()
    one = alone(ids_b, m)
    h0, vis = predicted_rows(nom, one, prm, vp, kind)
    if not vis.any():
        return None
    y = measured_rows(one, left_b, right_b, prm, kind)
    H = np.zeros((len(h0), 6))
    for j in range(6):
        col = []
        for s in (1.0, -1.0):
            d = np.zeros(6); d[j] = s * eps
            x = nom.copy()
            x[0:3] += d[0:3]
            x[6:10] = synth.qmul(nom[6:10][None], aa2q(d[3:6])[None])[0]
            col.append(predicted_rows(x, one, prm, vp, kind)[0])
        H[:, j] = (col[0] - col[1]) / (2 * eps)
    H, r = H[vis], (y - h0)[vis]
    Rn = r_meas if r_meas is not None else (prm.r_pos if kind == "corners" else prm.r_pix)
    S = H @ P[np.ix_(J, J)] @ H.T + Rn * np.eye(len(r))
    return float(r @ np.linalg.solve(S, r)), len(r), float(r @ r / Rn)


def pose_slot(orc, nom, rot, P, mid, yp, yq, prm, dialect):
    """(nis, dof, sum r^2 / R) of one marker's 7 pose rows (Matlab dialect: the oracle zeroes the quaternion residual, dof 3); None for
    an id that is not in the map"""
    if not in_map([mid], prm)[0]:
        return None
    _, H, r = orc.measurement(nom, rot, int(mid), np.asarray(yp, np.float64), np.asarray(yq, np.float64))
    Rd = np.array([prm.r_pos] * 3 + [prm.r_quat] * 4)
    S = H @ P @ H.T + np.diag(Rd)
    return float(r @ np.linalg.solve(S, r)), 7 if dialect == 1 else 3, float(np.sum(r * r / Rd))


def decide(ids, judged, nis, dof, thr, prm, skip=None):
    """(ids_out, kept) of the header's rules 4 from reported values: a judged slot is kept iff nis <= thr[dof] (a NaN is dropped)"""
    with np.errstate(invalid="ignore"):
        drop = judged & ~(nis <= np.asarray(thr, np.float64)[dof])
    ids_out = np.where(drop, -1, ids).astype(np.int32)
    kept = in_map(ids_out, prm).sum(axis=1).astype(np.int32)
    if skip is not None:
        kept[np.asarray(skip) != 0] = 0
    return ids_out, kept


def screen(state, ids, a, b, prm, kind, filters=None, dialect=0, nstate=18, skip=None, vp=None):
    """the statistic of every slot of the filters `filters` (default: all) -> nis (B, M) float64, dof (B, M) int32, judged (B, M) bool,
    rr (B, M) = sum r^2 / R; rows of the other filters are zero.  state: get_state() arrays.  kind "pose": a, b = pos, quat"""
    nom, rot, P = (np.asarray(x, np.float64) for x in state[:3])
    Bn, M = ids.shape
    nis, dof, judged, rr = np.zeros((Bn, M)), np.zeros((Bn, M), np.int32), np.zeros((Bn, M), bool), np.zeros((Bn, M))
    orc = oc.Oracle(dialect, nstate) if kind == "pose" else None
    for k in (range(Bn) if filters is None else filters):
        if skip is not None and skip[k]:
            continue
        for m in range(M):
            if kind == "pose":
                out = pose_slot(orc, nom[k], rot[k], P[k], ids[k, m], a[k, m], b[k, m], prm, dialect)
            else:
                out = image_slot(nom[k], P[k], ids[k], a[k], None if b is None else b[k], prm, kind, m, vp=vp)
            if out is not None:
                nis[k, m], dof[k, m], rr[k, m] = out
                judged[k, m] = True
    return nis, dof, judged, rr
