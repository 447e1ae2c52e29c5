"""fp64 numpy restatement of the general linearised measurement update (include/fbus_ekf.h, fbus_ekf_correct_rows), for the tests only:
written from the header's definition on ekf_oracle_np.State, not from the device code.  The caller's residual (m,) and dense H (m x N), S,
K = P H' S^-1, the injection exactly as ekf_oracle_np.correct has it, P in the oracle's literal form (I - K H) P or, on request, in its
Joseph form; the usable, pivot and gate rules of the header.  Also the other forms of the same update (P - U S^-1 U', m sequential rank-1
steps) for the CPU suite.  Never imported by the product package."""
import numpy as np

import ekf_oracle_np as E

ROWS_MAX = 3


def usable(res, H, var, skip=False):
    """not skipped, every residual and every entry of H finite, every variance a finite number > 0"""
    res, H, var = np.asarray(res, np.float64), np.asarray(H, np.float64), np.asarray(var, np.float64)
    return (not skip) and bool(np.isfinite(res).all()) and bool(np.isfinite(H).all()) and bool(np.isfinite(var).all()) \
        and bool((var > 0.0).all())


def pivots_of(S):
    """the squares of the Cholesky pivots of the m x m matrix S (the s_k of the sequential form), without a square root"""
    A = np.array(S, np.float64)
    out = []
    for k in range(len(A)):
        d = A[k, k]
        out.append(d)
        with np.errstate(all="ignore"):
            A = A - np.outer(A[:, k], A[k, :]) / d
    return np.array(out)


def correct_rows(s, n, res, H, var, thr=np.inf, skip=False, joseph=False):
    """One update of state s (modified in place when applied) by the rows H (m, n) with the innovation res (m,) and the variances var (m,).
    Returns (applied, nis, dof, lndetS): an unusable filter is left alone with (False, 0.0, 0, nan); a pivot that is not > 0 or
    nis > thr (or NaN) leaves it alone with (False, nis, m, lndetS)."""
    res, var = np.atleast_1d(np.asarray(res, np.float64)), np.atleast_1d(np.asarray(var, np.float64))
    H = np.asarray(H, np.float64).reshape(len(res), n)
    m = len(res)
    assert 1 <= m <= ROWS_MAX and var.shape == (m,)
    if not usable(res, H, var, skip):
        return False, 0.0, 0, float("nan")
    Rm = np.diag(var)
    S = H @ s.P @ H.T + Rm
    piv = pivots_of(S)
    with np.errstate(all="ignore"):
        nis = float(res @ np.linalg.solve(S, res)) if np.isfinite(S).all() else float("nan")
        lndet = float(np.log(piv).sum())
    if not ((piv > 0.0).all() and nis <= thr):
        return False, nis, m, lndet
    K = s.P @ H.T @ np.linalg.inv(S)                    # (n, m)
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
    return True, nis, m, lndet


def joint(P, H, var):
    """P - U S^-1 U' with U = P H'"""
    U = P @ H.T
    return P - U @ np.linalg.solve(H @ U + np.diag(var), U.T)


def sequential(P, H, var, res):
    """the m rank-1 steps at the one linearisation point -> (P, dx, nis, sum ln s_k, the s_k)"""
    P = np.array(P, np.float64)
    dx, nis, lnd, ss = np.zeros(len(P)), 0.0, 0.0, []
    for k in range(len(H)):
        u = P @ H[k]
        sk = H[k] @ u + var[k]
        rk = res[k] - H[k] @ dx
        dx = dx + u * rk / sk
        P = P - np.outer(u, u) / sk
        nis, lnd = nis + rk * rk / sk, lnd + np.log(sk)
        ss.append(sk)
    return P, dx, nis, lnd, np.array(ss)


def update_batch(st, n, res, H, var, thr=np.inf, skip=None, joseph=False):
    """correct_rows on every filter of get_state() arrays: res (B, m), H (B, m, n), var (m,) or (B, m) ->
    ((nominal, rot, P, prev), applied, nis, dof, ln det S)"""
    import velocity_ref as V
    ss = V.states_of(st, n)
    res, H = np.asarray(res, np.float64), np.asarray(H, np.float64)
    var = np.broadcast_to(np.asarray(var, np.float64), res.shape)
    out = [correct_rows(s, n, res[b], H[b], var[b], thr, bool(skip[b]) if skip is not None else False, joseph) for b, s in enumerate(ss)]
    app, nis, dof, lnd = (np.array(c) for c in zip(*out))
    return V.arrays_of(ss), app, nis, dof.astype(np.int32), lnd


# ---- the acoustic position fix of the re-acquisition cells (tests/test_rows_cpu.py, tests/test_rows_gpu.py) ------------------------------------
FIX = dict(lever=np.array([0.21, -0.08, 0.12]), var=np.array([1e-4, 4e-4, 2.5e-5]))        # a 1-2 cm fix: the depth suite's variance


def fix_inputs(st, dtype, n, seed=5):
    """get_state() arrays -> (res (B, 3), H (B, 3, n)) of fbus_ekf.rows.position_fix in the record type, for the reading
    z = h(state) + N(0, diag(FIX var)) rounded to the record type.  The rows do not depend on P."""
    import torch
    from fbus_ekf import rows
    t = np.float32 if dtype == 32 else np.float64
    nom, rot = np.asarray(st[0], np.float64), np.asarray(st[1], np.float64).reshape(-1, 3, 3)
    z = nom[:, 0:3] + rot @ FIX["lever"] + np.random.default_rng(seed).normal(0, 1, (len(nom), 3)) * np.sqrt(FIX["var"])
    res, H = rows.position_fix(torch.from_numpy(np.ascontiguousarray(st[0], t)), torch.from_numpy(np.ascontiguousarray(st[1], t)),
                               torch.from_numpy(z.astype(t)), FIX["lever"], nstate=n)
    return res.numpy(), H.numpy()
