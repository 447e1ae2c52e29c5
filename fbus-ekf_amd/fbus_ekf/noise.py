"""Per-filter noise tables for BatchedFilter.set_noise (fbus_ekf_set_noise): one row per filter, the columns below.

A noise sweep evaluates G hypotheses on one recording in one batch: noise.grid builds the Cartesian product of per-column
scale factors around a parameter set and assigns it to the filters round-robin (filter b gets hypothesis b mod G), so every
hypothesis is run by B / G filters.  noise.best is the other half: the per-hypothesis sum of the filters' innovation log-likelihood
(BatchedFilter.loglik) and its arg max -- NIS cannot rank hypotheses (it falls as the noise grows), the evidence can.
noise.group_weights is the numpy twin of the weights BatchedFilter.group_fuse forms on the device for contiguous groups of G filters
(the layout grid produces when G divides B); noise.imm_transition builds the model-transition matrix BatchedFilter.group_mix takes and
noise.group_mix_weights is the numpy twin of the mixing weights it forms.  numpy only.
"""
import itertools

import numpy as np

# the fbus_params fields, in the table's column order (FBUS_NOISE_COLS = 7)
COLUMNS = ("q_v", "q_theta", "q_ba", "q_bg", "r_pos", "r_quat", "r_pix")


def row_of(params):
    """the parameters' own values as one table row (q_diag[0..3], r_pos, r_quat, r_pix)"""
    q = list(params.q_diag)
    return np.array([q[0], q[1], q[2], q[3], params.r_pos, params.r_quat, params.r_pix], np.float64)


def from_params(params, B):
    """(B, 7): every filter with the parameters' own noise (the table that changes nothing)"""
    return np.tile(row_of(params), (int(B), 1))


def grid(params, B, **scales):
    """Cartesian product of per-column scale factors, e.g. grid(prm, B, r_pix=[0.5, 1, 2], q_v=[0.1, 1, 10]) -> 9 hypotheses.
    Columns not named keep the parameters' value.  Returns (table (B, 7), hyp (B,) int, rows (G, 7)): filter b runs hypothesis
    hyp[b] = b mod G, whose row is rows[hyp[b]]; the hypotheses are ordered as itertools.product over the named columns in
    COLUMNS order."""
    unknown = set(scales) - set(COLUMNS)
    if unknown:
        raise ValueError(f"grid: unknown columns {sorted(unknown)}; expected some of {COLUMNS}")
    base = row_of(params)
    named = [c for c in COLUMNS if c in scales]
    factors = [np.asarray(scales[c], np.float64).ravel() for c in named]
    rows = []
    for combo in itertools.product(*factors):
        r = base.copy()
        for c, f in zip(named, combo):
            r[COLUMNS.index(c)] *= f
        rows.append(r)
    rows = np.array(rows, np.float64).reshape(-1, len(COLUMNS))
    hyp = np.arange(int(B)) % len(rows)
    return rows[hyp], hyp, rows


def best(ll, hyp, G):
    """The evidence of each hypothesis and the winner: total[g] = sum of ll over the filters with hyp == g (a hypothesis no filter
    runs has total -inf and cannot win), g_best = the first arg max.  Returns (g_best, total (G,) float64)."""
    ll = np.asarray(ll, np.float64).ravel()
    hyp = np.asarray(hyp).ravel()
    G = int(G)
    if ll.shape != hyp.shape:
        raise ValueError(f"best: ll has {ll.size} entries, hyp {hyp.size}")
    if G < 1 or (hyp.size and (hyp.min() < 0 or hyp.max() >= G)):
        raise ValueError(f"best: hyp must lie in [0, {G})")
    total = np.full(G, -np.inf, np.float64)
    for g in range(G):
        sel = hyp == g
        if sel.any():
            total[g] = ll[sel].sum()
    return int(np.argmax(total)), total


def group_weights(logw, G):
    """The evidence weights of contiguous groups of G filters (steps 1-2 of fbus_ekf_group_fuse, include/fbus_ekf.h): group j holds
    filters j G .. j G + G - 1.  A member is usable iff its logw is finite (NaN, +inf and -inf exclude it, with weight exactly 0);
    with m the largest usable logw of the group, w_i = exp(logw_i - m) / sum exp(logw_k - m), summed in member order, and best is the
    first member with logw == m.  A group without a usable member has weights 0 and best -1.
    Returns (weight (B,) float64, best (B / G,) int32)."""
    lw = np.asarray(logw, np.float64).ravel()
    G = int(G)
    if G < 1 or lw.size % G:
        raise ValueError(f"group_weights: {lw.size} entries are not groups of {G}")
    lw = lw.reshape(-1, G)
    weight = np.zeros(lw.shape, np.float64)
    best = np.full(lw.shape[0], -1, np.int32)
    for j, row in enumerate(lw):
        ok = np.isfinite(row)
        if not ok.any():
            continue
        m = row[ok].max()
        best[j] = int(np.flatnonzero(ok & (row == m))[0])
        e = np.zeros(G, np.float64)
        e[ok] = np.exp(row[ok] - m)
        s = 0.0
        for v in e:
            s += v
        weight[j] = e / s
    return weight.ravel(), best


def imm_transition(G, stay):
    """The model-transition matrix of an IMM bank of G models that keeps its model with probability `stay` and moves to each of the
    others with equal probability: (G, G) float64, trans[i][j] = the probability that model i is followed by model j, `stay` on the
    diagonal and (1 - stay) / (G - 1) elsewhere (every row sums to 1)."""
    G, stay = int(G), float(stay)
    if G < 2 or not 0.0 <= stay <= 1.0:
        raise ValueError(f"imm_transition: G = {G} must be >= 2 and stay = {stay} a probability")
    trans = np.full((G, G), (1.0 - stay) / (G - 1), np.float64)
    trans[np.arange(G), np.arange(G)] = stay
    return trans


def check_transition(trans, G):
    """trans as a contiguous (G, G) float64 array, refused by the rule of the host form of fbus_ekf_group_mix: every entry finite and
    >= 0, every row sum within 1e-9 of 1.  The message names the row."""
    t = np.ascontiguousarray(trans, np.float64)
    G = int(G)
    if t.shape != (G, G):
        raise ValueError(f"trans: expected ({G}, {G}), got {t.shape}")
    for i, row in enumerate(t):
        if not np.isfinite(row).all() or (row < 0).any():
            raise ValueError(f"trans: row {i} has an entry that is not finite or is negative")
        s = 0.0
        for v in row:
            s += v
        if abs(s - 1.0) > 1e-9:
            raise ValueError(f"trans: row {i} sums to {s!r}, not to 1")
    return t


def group_mix_weights(logw, trans, G):
    """The mixing weights of contiguous groups of G filters (steps 1-2 of fbus_ekf_group_mix, include/fbus_ekf.h): mu = group_weights(logw),
    c_j = sum_i trans[i][j] mu_i summed in member order, W_ij = trans[i][j] mu_i / c_j -- the weight of source i in target j.  A target
    with c_j == 0 (every group without a usable member among them) has logc = -inf and a zero column of W.
    Returns (weight (B,) float64, logc (B,) float64, W (B / G, G, G) float64 indexed [group, i, j])."""
    G = int(G)
    trans = check_transition(trans, G)
    weight, _ = group_weights(logw, G)
    mu = weight.reshape(-1, G)
    logc = np.full(mu.shape, -np.inf, np.float64)
    W = np.zeros((mu.shape[0], G, G), np.float64)
    for g, row in enumerate(mu):
        for j in range(G):
            c = 0.0
            for i in range(G):
                c += trans[i, j] * row[i]
            if c > 0.0:
                logc[g, j] = np.log(c)
                W[g, :, j] = trans[:, j] * row / c
    return weight, logc.ravel(), W
