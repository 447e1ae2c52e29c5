"""Numpy restatement of fbus_ekf_sample (include/fbus_ekf.h), for the tests only: written from the header's contract, not from the device
code.  L = the lower Cholesky factor of Pi P Pi' (Pi: the error state p v theta ba bg [g] brought into the order p theta v ba bg [g]),
delta = Pi' L xi, then the injection: plain sums and q (x) dq(delta_theta), normalised.  The same formulas run in np.float64 and in
np.longdouble (`dtype`): the gap between the two is what the device tests take their tolerances from.
Never imported by the product package."""
import numpy as np

import nees_ref
from fbus_ekf import synth


def order(N):
    """position k of the factorisation order holds state order(N)[k] of the error state"""
    return [0, 1, 2, 6, 7, 8, 3, 4, 5] + list(range(9, N))


def factor(P, dtype=np.float64):
    """(L (B, N, N), ok (B,)): L L' = Pi P Pi' column by column in `dtype`, ok = all N pivots are > 0 (false for NaN).  Behind a bad pivot
    the entries are NaN."""
    P = np.asarray(P)
    B, N = P.shape[0], P.shape[1]
    o = order(N)
    A = P[:, o][:, :, o].astype(dtype)
    L = np.zeros((B, N, N), dtype)
    ok = np.ones(B, bool)
    with np.errstate(all="ignore"):
        for j in range(N):
            s = A[:, j, j] - np.einsum("bk,bk->b", L[:, j, :j], L[:, j, :j])
            ok &= s > 0
            d = np.sqrt(np.where(s > 0, s, dtype(np.nan)))
            L[:, j, j] = d
            for i in range(j + 1, N):
                L[:, i, j] = (A[:, i, j] - np.einsum("bk,bk->b", L[:, i, :j], L[:, j, :j])) / d
    return L, ok


def delta(P, xi, dtype=np.float64):
    """(delta (S, B, N) in error-state order, ok (B,)): Pi' L xi_s, xi (S, B, N) in the factorisation order"""
    L, ok = factor(P, dtype)
    N = L.shape[1]
    with np.errstate(all="ignore"):
        df = np.einsum("bij,sbj->sbi", L, np.asarray(xi, np.float64).astype(dtype))
    d = np.empty_like(df)
    d[:, :, order(N)] = df
    return d, ok


def inject(nominal, dx, dtype=np.float64):
    """(B, 19) in `dtype`: nominal (B, 19, taken as float64) (+) dx (B, N): one addition per plain component, q (x) dq normalised; for
    N = 15 g stays the nominal's"""
    x = np.asarray(nominal, np.float64).astype(dtype)
    dx = np.asarray(dx).astype(dtype)
    t = x.copy()
    with np.errstate(all="ignore"):
        t[:, 0:3] = x[:, 0:3] + dx[:, 0:3]
        t[:, 3:6] = x[:, 3:6] + dx[:, 3:6]
        t[:, 10:13] = x[:, 10:13] + dx[:, 9:12]
        t[:, 13:16] = x[:, 13:16] + dx[:, 12:15]
        if dx.shape[1] == 18:
            t[:, 16:19] = x[:, 16:19] + dx[:, 15:18]
        th = dx[:, 6:9]
        n = np.sqrt(th[:, 0] * th[:, 0] + th[:, 1] * th[:, 1] + th[:, 2] * th[:, 2])
        half = dtype(0.5) * n
        k = np.where(n == 0, dtype(0), np.sin(half) / np.where(n == 0, dtype(1), n))
        dq = np.concatenate([np.where(n == 0, dtype(1), np.cos(half))[:, None], k[:, None] * th], axis=1)
        q = synth.qmul(x[:, 6:10], dq)
        t[:, 6:10] = q / np.sqrt(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3])[:, None]
    return t


def sample(nominal, P, xi, skip=None, dtype=np.float64):
    """(state (S, B, 19) in `dtype`, drawn (B,) uint8, delta (S, B, N)) from get_state()'s nominal (B, 19) and P (B, N, N) and
    xi (S, B, N).  A filter that is skipped or not positive definite: drawn = 0 and every row its nominal as float64, unchanged."""
    d, ok = delta(P, xi, dtype)
    if skip is not None:
        ok = ok & (np.asarray(skip) == 0)
    x = np.asarray(nominal, np.float64).astype(dtype)
    out = np.stack([inject(nominal, d[s], dtype) for s in range(d.shape[0])])
    out[:, ~ok] = x[~ok]
    return out, ok.astype(np.uint8), d


def prefix_sums(xi):
    """(FULL, POSE, P), each (S, B): |xi|^2, |xi(0..5)|^2, |xi(0..2)|^2 in longdouble -- what fbus_ekf_nees returns for a drawn row"""
    x2 = np.asarray(xi, np.float64).astype(np.longdouble) ** 2
    return x2.sum(axis=2), x2[:, :, :6].sum(axis=2), x2[:, :, :3].sum(axis=2)


def loop(nominal, P, xi, rows=None, cast=None):
    """The closed loop of the reference in float64: every row of sample() (or `rows`) fed back as truth to nees_ref.nees.
    -> (cols (S, B, 3) = FULL, POSE, P, err (S, B, N)).  cast: a function applied to the rows first, which then are the ESTIMATE and
    `nominal` the truth (what perturb() followed by nees(truth) computes)"""
    if rows is None:
        rows = sample(nominal, P, xi)[0]
    cols, errs = [], []
    for s in range(len(rows)):
        if cast is None:
            n, e, _ = nees_ref.nees(nominal, P, rows[s])
        else:
            n, e, _ = nees_ref.nees(cast(rows[s]), P, np.asarray(nominal, np.float64))
        cols.append(n[:, [0, 1, 2]])
        errs.append(e)
    return np.stack(cols), np.stack(errs)


def moments(nominal, rows, w, N):
    """(mean (B, N), cov (B, N, N)) in longdouble: sum w delta and sum w delta delta' of the rows (S, B, 19) about `nominal`, delta by
    nees_ref.delta"""
    d = np.stack([nees_ref.delta(nominal, rows[s], N, np.longdouble) for s in range(len(rows))])
    w = np.asarray(w, np.float64).astype(np.longdouble)
    return np.einsum("s,sbi->bi", w, d), np.einsum("s,sbi,sbj->bij", w, d, d)


def moment_gaps(nominal, P, rows, w):
    """(largest |sum w delta|_i / sqrt(P_ii), largest |sum w delta delta' - P|_ij / sqrt(P_ii P_jj)) over the batch"""
    P = np.asarray(P, np.float64).astype(np.longdouble)
    N = P.shape[1]
    m, c = moments(nominal, rows, w, N)
    sd = np.sqrt(np.einsum("bii->bi", P))
    return float(np.max(np.abs(m) / sd)), float(np.max(np.abs(c - P) / (sd[:, :, None] * sd[:, None, :])))
