"""fp64 numpy restatement of fbus_ekf_group_mix (include/fbus_ekf.h, "hypothesis groups"), for the tests only: it works from get_state()
arrays, the log-weights and the transition matrix, one group at a time, in member order.  Never imported by the product package."""
import numpy as np

import group_ref
from group_ref import _PLAIN


def mix_weights(logw, trans):
    """steps 1-2 for ONE group: (mu (G,), best, c (G,), W (G, G) indexed [source i, target j]; a column with c_j == 0 is zero)"""
    trans = np.asarray(trans, np.float64)
    mu, best = group_ref.weights(logw)
    G = mu.size
    c, W = np.zeros(G), np.zeros((G, G))
    for j in range(G):
        for i in range(G):
            c[j] += trans[i, j] * mu[i]
        if best >= 0 and c[j] > 0.0:
            for i in range(G):
                W[i, j] = trans[i, j] * mu[i] / c[j]
    return mu, best, c, W


def mix_group(nominal, rot, P, logw, trans):
    """nominal (G, 19), rot (G, 9), P (G, N, N), logw (G,) of one group, trans (G, G) -> (mu, logc, nominal, rot, P) after the mix.  A
    target that is not rewritten (c_j == 0, W_jj == 1, no usable member) is returned as it came, bit for bit."""
    nominal, rot, P = (np.array(x, np.float64) for x in (nominal, rot, P))
    G, N = nominal.shape[0], P.shape[-1]
    mu, best, c, W = mix_weights(logw, trans)
    with np.errstate(divide="ignore"):
        logc = np.where((best >= 0) & (c > 0.0), np.log(c), -np.inf)
    if best < 0:
        return mu, logc, nominal, rot, P
    xs = nominal[best]
    out_nom, out_rot, out_P = nominal.copy(), rot.copy(), P.copy()
    dl = {i: group_ref.delta(nominal[i], xs, N) for i in range(G) if W[i].any()}
    for j in range(G):
        if not c[j] > 0.0 or W[j, j] == 1.0:
            continue
        use = [i for i in range(G) if W[i, j] != 0.0]      # a weightless source is skipped, not multiplied by 0
        m = np.zeros(N)
        for i in use:
            m = m + W[i, j] * dl[i]
        x = xs.copy()
        for a, b, o in _PLAIN:
            if o < N:
                x[a:b] = xs[a:b] + m[o:o + 3]
        q = group_ref.qmul(xs[6:10], group_ref.dq(m[6:9]))
        x[6:10] = q / np.linalg.norm(q)
        Pj = np.zeros((N, N))
        for i in use:
            d = dl[i] - m
            Pj = Pj + W[i, j] * (P[i] + np.outer(d, d))
        out_nom[j], out_rot[j], out_P[j] = x, rot[best], Pj
    return mu, logc, out_nom, out_rot, out_P


def mix(state, logw, trans, G):
    """the whole batch: state = (nominal (B, 19), rot (B, 9), P (B, N, N), ...) as get_state() returns it -> (weight (B,), logc (B,),
    nominal, rot, P) after the mix"""
    nominal, rot, P = (np.array(x, np.float64) for x in state[:3])
    B = nominal.shape[0]
    assert B % G == 0
    logw = np.asarray(logw, np.float64)
    weight, logc = np.zeros(B), np.zeros(B)
    for g in range(B // G):
        s = slice(g * G, (g + 1) * G)
        weight[s], logc[s], nominal[s], rot[s], P[s] = mix_group(nominal[s], rot[s], P[s], logw[s], trans)
    return weight, logc, nominal, rot, P
