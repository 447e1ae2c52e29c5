"""fp64 numpy restatement of fbus_ekf_group_fuse (include/fbus_ekf.h, "hypothesis groups"), for the tests only: it works from
get_state() arrays and the log-weights, one group at a time, in member order.  Never imported by the product package."""
import numpy as np

# API nominal order p v q ba bg g  ->  error-state order p v theta ba bg [g]
_PLAIN = ((0, 3, 0), (3, 6, 3), (10, 13, 9), (13, 16, 12), (16, 19, 15))      # (nominal from, to, error-state from)


def qmul(p, q):
    pw, px, py, pz = p
    qw, qx, qy, qz = q
    return np.array([pw * qw - px * qx - py * qy - pz * qz,
                     pw * qx + px * qw + py * qz - pz * qy,
                     pw * qy - px * qz + py * qw + pz * qx,
                     pw * qz + px * qy - py * qx + pz * qw])


def log_q(qs, q):
    """dtheta = Log(conj(q*) (x) q): the inverse of q <- normalize(q* (x) dq(dtheta))"""
    d = qmul(np.array([qs[0], -qs[1], -qs[2], -qs[3]]), q)
    if d[0] < 0:
        d = -d
    n = np.sqrt(d[1] * d[1] + d[2] * d[2] + d[3] * d[3])
    if n == 0:
        return np.zeros(3)
    return (2.0 * np.arctan2(n, d[0]) / n) * d[1:]


def dq(theta):
    """the injection's rotation increment (MeasureUpdate.m:92-98): axis-angle -> quaternion"""
    n = np.linalg.norm(theta)
    if n == 0:
        return np.array([1.0, 0.0, 0.0, 0.0])
    return np.concatenate([[np.cos(0.5 * n)], np.sin(0.5 * n) / n * theta])


def weights(logw):
    """steps 1-2 for ONE group: (w (G,), best)"""
    lw = np.asarray(logw, np.float64)
    G = lw.size
    ok = np.isfinite(lw)
    if not ok.any():
        return np.zeros(G), -1
    m = max(lw[i] for i in range(G) if ok[i])
    best = next(i for i in range(G) if ok[i] and lw[i] == m)
    e = [np.exp(lw[i] - m) if ok[i] else 0.0 for i in range(G)]
    s = 0.0
    for i in range(G):
        if ok[i]:
            s += e[i]
    return np.array([e[i] / s if ok[i] else 0.0 for i in range(G)]), best


def delta(x, xs, N):
    """one member's error state against the chart xs"""
    d = np.zeros(N)
    for a, b, o in _PLAIN:
        if o < N:
            d[o:o + 3] = x[a:b] - xs[a:b]
    d[6:9] = log_q(xs[6:10], x[6:10])
    return d


def fuse_group(nominal, P, logw):
    """nominal (G, 19), P (G, N, N), logw (G,) of one group -> (w, best, fused nominal (19,), fused P (N, N))"""
    nominal = np.asarray(nominal, np.float64)
    P = np.asarray(P, np.float64)
    G, N = nominal.shape[0], P.shape[-1]
    w, best = weights(logw)
    if best < 0:
        return w, best, nominal[0].copy(), P[0].copy()
    xs = nominal[best]
    use = [i for i in range(G) if w[i] != 0.0]              # a weightless member is skipped, not multiplied by 0
    dl = {i: delta(nominal[i], xs, N) for i in use}
    mu = np.zeros(N)
    for i in use:
        mu = mu + w[i] * dl[i]
    out = xs.copy()
    for a, b, o in _PLAIN:
        if o < N:
            out[a:b] = xs[a:b] + mu[o:o + 3]
    q = qmul(xs[6:10], dq(mu[6:9]))
    out[6:10] = q / np.linalg.norm(q)
    Pb = np.zeros((N, N))
    for i in use:
        d = dl[i] - mu
        Pb = Pb + w[i] * (P[i] + np.outer(d, d))
    return w, best, out, Pb


def fuse(nominal, P, logw, G):
    """the whole batch: (weight (B,), best (B/G,), nominal (B/G, 19), P (B/G, N, N))"""
    nominal = np.asarray(nominal, np.float64).reshape(-1, 19)
    B, N = nominal.shape[0], np.asarray(P).shape[-1]
    assert B % G == 0
    NG = B // G
    weight, best = np.zeros(B), np.zeros(NG, np.int32)
    nom, Pb = np.zeros((NG, 19)), np.zeros((NG, N, N))
    for j in range(NG):
        s = slice(j * G, (j + 1) * G)
        weight[s], best[j], nom[j], Pb[j] = fuse_group(nominal[s], np.asarray(P)[s], np.asarray(logw, np.float64)[s])
    return weight, best, nom, Pb
