"""fp64 numpy restatement of the depth (pressure) sensor update (include/fbus_ekf.h, fbus_ekf_correct_depth), for the tests only: written
from the header's definition on ekf_oracle_np.State, not from the device code.  Dense H (1 x N), S, K = P H' / S, the injection exactly as
ekf_oracle_np.correct has it, P in the oracle's literal form (I - K H) P or, on request, in its Joseph form.  Never imported by the
product package."""
import numpy as np

import ekf_oracle_np as E


def unit(axis):
    a = np.asarray(axis, np.float64)
    return a / np.sqrt(a @ a)                  # (as the host normalises it: a / sqrt(a0^2 + a1^2 + a2^2) in double)


def lever_of(lever):
    return np.zeros(3) if lever is None else np.asarray(lever, np.float64)


def h(s, axis, offset, lever):
    """the predicted reading of state s; axis already a unit vector.  s.R is the CARRIED rotation"""
    return float(axis @ (s.p + s.R @ lever) + offset)


def H_row(s, n, axis, lever):
    """(1, n): columns 0..2 = axis', columns 6..8 = (lever x (R' axis))', every other column 0"""
    H = np.zeros((1, n))
    H[0, 0:3] = axis
    H[0, 6:9] = np.cross(lever, s.R.T @ axis)
    return H


def usable(z, var, skip=False):
    return (not skip) and bool(np.isfinite(z)) and bool(np.isfinite(var)) and var > 0.0


def correct_depth(s, n, z, var, axis, offset=0.0, lever=None, thr1=np.inf, skip=False, joseph=False):
    """One depth update of state s (modified in place when applied).  axis: as handed to fbus_ekf_set_depth_sensor (normalised here).
    Returns (applied, nis, dof, S): a skipped filter, a non-finite z and a var that is not a finite number > 0 leave the state alone with
    (False, 0.0, 0, nan); the update is applied iff S > 0 and nis <= thr1 (both comparisons false for a NaN: the rule of
    velocity_ref.correct_velocity and rows_ref.correct_rows with S the one pivot), anything else leaves it alone with
    (False, nis, 1, S)."""
    if not usable(z, var, skip):
        return False, 0.0, 0, float("nan")
    a, lv = unit(axis), lever_of(lever)
    H = H_row(s, n, a, lv)
    res = float(z) - h(s, a, offset, lv)
    S = (H @ s.P @ H.T).item() + float(var)
    with np.errstate(all="ignore"):
        nis = res * res / S
    if not (S > 0.0 and nis <= thr1):
        return False, nis, 1, S
    K = s.P @ H.T / S                                   # (n, 1)
    dx = (K * res).ravel()
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
        P = P @ IKH.T + K * var @ K.T
    s.P = (P + P.T) / 2
    return True, nis, 1, S


def rank1(P, H, var):
    """P - u u' / S with u = P H': the form the kernel applies"""
    u = P @ H.T
    return P - (u @ u.T) / ((H @ u).item() + var)
