"""The dense references of the innovation log-likelihood terms of the pose, pixel and corner updates (include/fbus_ekf.h, "per-filter
innovation log-likelihood"): S exactly as nis_reference / pose_nis_reference of tests/test_nis_gpu.py build it, and the tolerance on -2 ll
that goes with them.  tests/test_loglik_gpu.py holds one update to them, tests/cycle_ref.py composes them into the IMM cycle.  A plain
library: no tests and no pytest marks, importable without a GPU."""
import math

import numpy as np

import oracle_capi as oc
from fbus_ekf import synth
from support import J, aa2q, measured_rows, predicted_rows

LN2PI = math.log(2.0 * math.pi)


def dense_pixels(nom, P, ids_b, left_b, right_b, prm, kind, r=None, eps=1e-6, vp=None):
    """(nis, log det S, rows, ln r) of one filter's pixel / corner rows; r: this filter's R (default: the parameters')"""
    vp = vp if vp is not None else oc.vision_params()
    h0, vis = predicted_rows(nom, ids_b, prm, vp, kind)
    y = measured_rows(ids_b, left_b, right_b, prm, kind)
    H = np.zeros((len(h0), 6))
    for j in range(6):
        col = []
        for s in (1.0, -1.0):
            d = np.zeros(6); d[j] = s * eps
            x = nom.copy()
            x[0:3] += d[0:3]
            x[6:10] = synth.qmul(nom[6:10][None], aa2q(d[3:6])[None])[0]
            col.append(predicted_rows(x, ids_b, prm, vp, kind)[0])
        H[:, j] = (col[0] - col[1]) / (2 * eps)
    H, res = H[vis], (y - h0)[vis]
    Rn = r if r is not None else (prm.r_pos if kind == "corners" else prm.r_pix)
    S = H @ P[np.ix_(J, J)] @ H.T + Rn * np.eye(len(res))
    sign, ld = np.linalg.slogdet(S)
    assert sign > 0
    return float(res @ np.linalg.solve(S, res)), float(ld), len(res), math.log(Rn)


def dense_pose(orc, nom, rot, P, ids_b, pos_b, quat_b, used_ids, prm):
    """(nis, log det S, rows, rr) over all 7 rows of each used marker (Matlab dialect: the oracle's quaternion residual is zero,
    its rows stay in S)"""
    Hs, rs = [], []
    for m, mid in enumerate(ids_b):
        if mid not in used_ids:
            continue
        _, H, r = orc.measurement(nom, rot, int(mid), pos_b[m], quat_b[m])
        Hs.append(H); rs.append(r)
    H, r = np.concatenate(Hs), np.concatenate(rs)
    Rd = np.tile(np.array([prm.r_pos] * 3 + [prm.r_quat] * 4), len(rs))
    S = H @ P @ H.T + np.diag(Rd)
    sign, ld = np.linalg.slogdet(S)
    assert sign > 0
    return float(r @ np.linalg.solve(S, r)), float(ld), len(r), float(np.sum(r * r / Rd))


def tol_m2ll(dtype, pose, nis_ref, ld_ref, rr=0.0):
    """the tolerance on -2 ll: the NIS tolerance of the route (tests/test_nis_gpu.py) plus the log-determinant term -- fp32: 1e-4
    absolute (ln r is formed in double from a double, P_JJ is read back exactly; what is left is the pose fold's Lam in fp32, <= 64
    roundings of 2^-24 per entry, and |d log det(I + P Lam)| <= 6 |d Lam| / |Lam|: 2.3e-5, gate at 4 x); fp64: the NIS figure of the
    route times max(|log det S|, 1)"""
    if pose:
        t = (1e-3 * max(nis_ref, 1.0) + 1e-6 * rr) if dtype == 32 else (1e-8 * max(nis_ref, 1.0) + 1e-12 * rr)
        return t + (1e-4 if dtype == 32 else 1e-8 * max(abs(ld_ref), 1.0))
    t = (1e-3 if dtype == 32 else 1e-6) * max(nis_ref, 1.0)
    return t + (1e-4 if dtype == 32 else 1e-6 * max(abs(ld_ref), 1.0))
