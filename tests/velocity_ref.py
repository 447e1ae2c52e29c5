"""fp64 numpy restatement of the body-velocity (DVL) update (include/fbus_ekf.h, fbus_ekf_correct_velocity), for the tests only: written
from the header's definition on ekf_oracle_np.State, not from the device code.  Dense H (3 x N), S, K = P H' S^-1, the injection exactly
as ekf_oracle_np.correct has it, P in the oracle's literal form (I - K H) P or, on request, in its Joseph form; the usable, pivot and gate
rules of the header.  Also the other forms of the same update (P - U S^-1 U', three sequential rank-1 steps) for the CPU suite, and the
conversions between get_state() arrays and oracle states.  Never imported by the product package."""
import numpy as np

import ekf_oracle_np as E


def mount_of(mount):
    return np.eye(3) if mount is None else np.asarray(mount, np.float64).reshape(3, 3)


def lever_of(lever):
    return np.zeros(3) if lever is None else np.asarray(lever, np.float64)


def tilted_mount():
    """a rotation with no zero entry: 0.3 rad about (1, -2, 3) / sqrt(14)"""
    a = np.array([1.0, -2.0, 3.0]) / np.sqrt(14.0)
    K = E.skew(a)
    return np.eye(3) + np.sin(0.3) * K + (1 - np.cos(0.3)) * (K @ K)


def states_of(st, n):
    """get_state() arrays -> one ekf_oracle_np.State per filter, in double"""
    nom, rot, P, prev = (np.asarray(x, np.float64) if i < 3 else np.asarray(x) for i, x in enumerate(st))
    out = []
    for b in range(len(nom)):
        s = E.State(n)
        s.p, s.v, s.q, s.ba, s.bg, s.g = (nom[b, a:e].copy() for a, e in ((0, 3), (3, 6), (6, 10), (10, 13), (13, 16), (16, 19)))
        s.R, s.P, s.prev_id = rot[b].reshape(3, 3).copy(), P[b].copy(), int(prev[b])
        out.append(s)
    return out


def arrays_of(states):
    nom = np.array([np.concatenate([s.p, s.v, s.q, s.ba, s.bg, s.g]) for s in states])
    return nom, np.array([s.R.ravel() for s in states]), np.array([s.P for s in states]), np.array([s.prev_id for s in states], np.int32)


def h(s, C, lever, gyro=None):
    """the predicted reading (3,) of state s: C (R' v + (gyro - bg) x lever); s.R is the CARRIED rotation.  gyro None: no lever term"""
    y = s.R.T @ s.v
    if gyro is not None:
        y = y + np.cross(np.asarray(gyro, np.float64) - s.bg, lever)
    return C @ y


def H_rows(s, n, C, lever, gyro=None):
    """(3, n): columns 3..5 = C R', 6..8 = C [R' v]x, 12..14 = C [lever]x (zero without gyro), every other column 0"""
    H = np.zeros((3, n))
    H[:, 3:6] = C @ s.R.T
    H[:, 6:9] = C @ E.skew(s.R.T @ s.v)
    if gyro is not None:
        H[:, 12:15] = C @ E.skew(lever)
    return H


def usable(z, var, gyro=None, skip=False):
    var = np.asarray(var, np.float64)
    ok = (not skip) and bool(np.isfinite(z).all()) and bool(np.isfinite(var).all()) and bool((var > 0.0).all())
    return ok and (gyro is None or bool(np.isfinite(gyro).all()))


def pivots_of(S):
    """the squares of the Cholesky pivots of the 3 x 3 matrix S (the s_k of the sequential form), without a square root"""
    A = np.array(S, np.float64)
    out = []
    for k in range(3):
        d = A[k, k]
        out.append(d)
        with np.errstate(all="ignore"):
            A = A - np.outer(A[:, k], A[k, :]) / d
    return np.array(out)


def correct_velocity(s, n, z, var, gyro=None, mount=None, lever=None, thr3=np.inf, skip=False, joseph=False):
    """One velocity update of state s (modified in place when applied).  Returns (applied, nis, dof, lndetS): a skipped filter, a
    non-finite z or gyro component and a variance that is not a finite number > 0 leave the state alone with (False, 0.0, 0, nan); a pivot
    that is not > 0 or nis > thr3 (or NaN) leaves it alone with (False, nis, 3, lndetS)."""
    z, var = np.asarray(z, np.float64), np.asarray(var, np.float64)
    if not usable(z, var, gyro, skip):
        return False, 0.0, 0, float("nan")
    C, lv = mount_of(mount), lever_of(lever)
    H = H_rows(s, n, C, lv, gyro)
    res = z - h(s, C, lv, gyro)
    Rm = np.diag(var)
    S = H @ s.P @ H.T + Rm
    piv = pivots_of(S)
    with np.errstate(all="ignore"):
        nis = float(res @ np.linalg.solve(S, res)) if np.isfinite(S).all() else float("nan")
        lndet = float(np.log(piv).sum())
    if not ((piv > 0.0).all() and nis <= thr3):
        return False, nis, 3, lndet
    K = s.P @ H.T @ np.linalg.inv(S)                    # (n, 3)
    dx = K @ res
    s.p = s.p + dx[0:3]
    s.v = s.v + dx[3:6]
    nrm = np.linalg.norm(dx[6:9])
    if nrm > 0:                                          # (ekf_oracle_np.correct divides by the norm: 0 / 0 where nothing turns)
        q = E.qmul(s.q, E.aa2q(dx[6:9], nrm))
        s.q = q / np.linalg.norm(q)
    s.ba = s.ba + dx[9:12]
    s.bg = s.bg + dx[12:15]
    if n == 18:
        s.g = s.g + dx[15:18]
    IKH = np.eye(n) - K @ H
    P = IKH @ s.P
    if joseph:
        P = P @ IKH.T + K @ Rm @ K.T
    s.P = (P + P.T) / 2
    return True, nis, 3, lndet


def joint(P, H, var):
    """P - U S^-1 U' with U = P H'"""
    U = P @ H.T
    return P - U @ np.linalg.solve(H @ U + np.diag(var), U.T)


def sequential(P, H, var, res):
    """the three rank-1 steps at the one linearisation point -> (P, dx, nis, sum ln s_k, the s_k)"""
    P = np.array(P, np.float64)
    dx, nis, lnd, ss = np.zeros(len(P)), 0.0, 0.0, []
    for k in range(3):
        u = P @ H[k]
        sk = H[k] @ u + var[k]
        rk = res[k] - H[k] @ dx
        dx = dx + u * rk / sk
        P = P - np.outer(u, u) / sk
        nis, lnd = nis + rk * rk / sk, lnd + np.log(sk)
        ss.append(sk)
    return P, dx, nis, lnd, np.array(ss)
