"""Numpy restatement of fbus_ekf_nees (include/fbus_ekf.h), for the tests only: written from the header's definition, not from the device
code.  delta = truth (-) estimate (step 3 of fbus_ekf_group_fuse with the estimate as the chart), every column of nees by a Cholesky
factorisation of ITS OWN marginal in the natural order of the error state, lnp from the full factorisation's pivots.  The same formulas run
in np.float64 and in np.longdouble (`dtype`): the gap between the two is what the device parity test takes its tolerance from.
Never imported by the product package."""
import numpy as np

from fbus_ekf import synth

COLS = 8
LN_2PI = 1.8378770664093454835606594728112352797227949472755668


def blocks(N):
    """the index sets of the 8 columns in the error-state order p v theta ba bg [g]; G is empty for N = 15"""
    return [list(range(N)), [0, 1, 2, 6, 7, 8], [0, 1, 2], [3, 4, 5], [6, 7, 8], [9, 10, 11], [12, 13, 14], [15, 16, 17] if N == 18 else []]


def delta(nominal, truth, N, dtype=np.float64):
    """(B, N): truth (-) estimate, both (B, 19) in get_state's order.  The plain components are one subtraction of the two values as
    doubles -- in every dtype, so that the float64 path is the device's bit for bit and the longdouble path starts from the same numbers"""
    x, t = np.asarray(nominal, np.float64), np.asarray(truth, np.float64)
    B = len(x)
    d = np.empty((B, N), dtype)
    with np.errstate(all="ignore"):
        d[:, 0:3] = t[:, 0:3] - x[:, 0:3]
        d[:, 3:6] = t[:, 3:6] - x[:, 3:6]
        d[:, 9:12] = t[:, 10:13] - x[:, 10:13]
        d[:, 12:15] = t[:, 13:16] - x[:, 13:16]
        if N == 18:
            d[:, 15:18] = t[:, 16:19] - x[:, 16:19]
        q, qt = x[:, 6:10].astype(dtype), t[:, 6:10].astype(dtype)
        qt = qt / np.sqrt(qt[:, 0] * qt[:, 0] + qt[:, 1] * qt[:, 1] + qt[:, 2] * qt[:, 2] + qt[:, 3] * qt[:, 3])[:, None]
        qc = q * np.array([1, -1, -1, -1], dtype)
        e = synth.qmul(qc, qt)                                  # conj(q) (x) q_true
        e = np.where((e[:, 0] < 0)[:, None], -e, e)
        n = np.sqrt(e[:, 1] * e[:, 1] + e[:, 2] * e[:, 2] + e[:, 3] * e[:, 3])
        k = np.where(n == 0, dtype(0), dtype(2) * np.arctan2(n, e[:, 0]) / np.where(n == 0, dtype(1), n))
        d[:, 6:9] = k[:, None] * e[:, 1:4]
    return d


def chol_solve(A, d):
    """A (B, n, n), d (B, n), any float dtype: (y, piv, bad) with L L' = A row by row, y = L^-1 d, piv the squared pivots L_ii^2 and
    bad (B,) = a pivot is not > 0 (false for NaN) or a component of d is not finite.  Behind a bad pivot the rows are NaN."""
    B, n = d.shape
    dt = d.dtype.type
    L = np.zeros((B, n, n), dt)
    y = np.zeros((B, n), dt)
    piv = np.zeros((B, n), dt)
    bad = ~np.isfinite(d).all(axis=1)
    with np.errstate(all="ignore"):
        for i in range(n):
            for j in range(i):
                s = A[:, i, j].astype(dt)
                for k in range(j):
                    s = s - L[:, i, k] * L[:, j, k]
                L[:, i, j] = s / L[:, j, j]
            s = A[:, i, i].astype(dt)
            for k in range(i):
                s = s - L[:, i, k] * L[:, i, k]
            piv[:, i] = s
            bad |= ~(s > 0)
            L[:, i, i] = np.sqrt(np.where(s > 0, s, dt(np.nan)))
            u = d[:, i]
            for k in range(i):
                u = u - L[:, i, k] * y[:, k]
            y[:, i] = u / L[:, i, i]
    return y, piv, bad


def block_nees(A, d):
    """d' A^-1 d = |L^-1 d|^2 per filter, NaN by the column rule"""
    y, _, bad = chol_solve(A, d)
    with np.errstate(all="ignore"):
        s = (y * y).sum(axis=1)
    return np.where(bad, d.dtype.type(np.nan), s)


def nees(nominal, P, truth, skip=None, dtype=np.float64):
    """(nees (B, 8), err (B, N), lnp (B,)) in `dtype` from get_state()'s nominal (B, 19) and P (B, N, N) and truth (B, 19)"""
    P = np.asarray(P)
    B, N = P.shape[0], P.shape[1]
    d = delta(nominal, truth, N, dtype)
    Pd = P.astype(dtype)
    out = np.zeros((B, COLS), dtype)
    for c, Jc in enumerate(blocks(N)):
        if Jc:
            out[:, c] = block_nees(Pd[:, Jc][:, :, Jc], d[:, Jc])
    _, piv, bad = chol_solve(Pd, d)
    with np.errstate(all="ignore"):
        lnp = dtype(-0.5) * (out[:, 0] + np.log(piv).sum(axis=1) + dtype(N) * dtype(LN_2PI))
    lnp = np.where(bad, dtype(np.nan), lnp)
    if skip is not None:
        s = np.asarray(skip) != 0
        out[s], d[s], lnp[s] = 0, 0, 0
    return out, d, lnp


def rel_gap(a, b):
    """the largest |a - b| / |b| over the entries where b is finite and not 0 (b: the better value)"""
    a, b = np.asarray(a, np.longdouble).ravel(), np.asarray(b, np.longdouble).ravel()
    m = np.isfinite(b) & (b != 0)
    return float(np.max(np.abs(a[m] - b[m]) / np.abs(b[m]))) if m.any() else 0.0


def path_gap(nominal, P, truth):
    """the largest relative gap between the float64 and the longdouble path on these inputs, over nees, err's theta entries and lnp"""
    n64, e64, l64 = nees(nominal, P, truth, dtype=np.float64)
    nld, eld, lld = nees(nominal, P, truth, dtype=np.longdouble)
    return max(rel_gap(n64, nld), rel_gap(e64[:, 6:9], eld[:, 6:9]), rel_gap(l64, lld))


# ---- the inputs of the tests --------------------------------------------------------------------------------------------------------
def boxplus(nominal, dx):
    """truth = estimate (+) dx in float64: plain sums and q (x) Exp(dx_theta), the injection's convention; dx (B, N) in error-state order.
    For N = 15 the truth's g is the estimate's (the call ignores it)."""
    x, dx = np.asarray(nominal, np.float64), np.asarray(dx, np.float64)
    t = x.copy()
    t[:, 0:3] += dx[:, 0:3]
    t[:, 3:6] += dx[:, 3:6]
    t[:, 10:13] += dx[:, 9:12]
    t[:, 13:16] += dx[:, 12:15]
    if dx.shape[1] == 18:
        t[:, 16:19] += dx[:, 15:18]
    th = np.linalg.norm(dx[:, 6:9], axis=1)
    half = 0.5 * th
    w = np.where(th == 0, 0.5, np.sin(half) / np.where(th == 0, 1.0, th))
    dq = np.concatenate([np.cos(half)[:, None], w[:, None] * dx[:, 6:9]], axis=1)
    t[:, 6:10] = synth.qmul(x[:, 6:10], dq)
    return t


def draw_dx(P, seed):
    """dx ~ N(0, P) per filter: L z with L = the float64 Cholesky factor of P (B, N, N), z from default_rng(seed)"""
    P = np.asarray(P, np.float64)
    z = np.random.default_rng(seed).normal(size=P.shape[:2])
    return np.einsum("bij,bj->bi", np.linalg.cholesky(P), z)


def calibration_inputs(n=8192, nstate=18, seed=1):
    """(nominal, rot, P, prev, truth): n filters of synth.initial_state(mixed_cov=True) with the covariance rounded to fp32, and
    truth = estimate (+) dx, dx ~ N(0, P) -- what the CPU and the device calibration tests share"""
    from fbus_ekf import capi
    prm = capi.default_params(0)
    nom, rot, P, prev = synth.initial_state(0, n, list(prm.p0_diag), nstate, mixed_cov=True)
    r32 = lambda a: np.asarray(a, np.float64).astype(np.float32).astype(np.float64)
    nom, rot, P = r32(nom), r32(rot), r32(P)
    return nom, rot, P, prev, boxplus(nom, draw_dx(P, seed))
