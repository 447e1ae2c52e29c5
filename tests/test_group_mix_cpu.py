"""CPU suite for the IMM mixing of hypothesis groups (include/fbus_ekf.h, fbus_ekf_group_mix; added under FBUS_ABI_VERSION 8 without a
bump): the two symbols and their null-handle checks, fbus_ekf.noise.imm_transition / group_mix_weights on hand-made arrays, and
tests/group_mix_ref.py -- the fp64 restatement the GPU suite holds the kernel to -- on the cases whose answer is known: the identity
matrix (nothing changes), a rank-one matrix (every target is group_ref.fuse_group's estimate) and a sticky matrix (proper covariances)."""
import ctypes as C
import os

import numpy as np
import pytest

import group_mix_ref
import group_ref
from fbus_ekf import capi, noise

NEW = ["fbus_ekf_group_mix", "fbus_ekf_group_mix_dev"]


def test_the_two_symbols_are_declared_exported_and_refuse_a_null_handle():
    declared = capi.declared_symbols()
    lib = capi.load_library()
    for n in NEW:
        assert n in declared, n
        assert hasattr(lib, n), n
    assert capi.ABI_VERSION == 8 and lib.fbus_ekf_abi_version() == 8
    w = (C.c_double * 4)()
    t = (C.c_double * 4)(1.0, 0.0, 0.0, 1.0)
    for fn in NEW:
        assert getattr(lib, fn)(None, 2, w, t, w, w) == 1
        assert getattr(lib, fn)(None, 2, None, None, None, None) == 1


def test_the_python_and_cxx_layers_carry_the_method(repo_root):
    from fbus_ekf import BatchedFilter
    assert callable(BatchedFilter.group_mix) and "logc = log prior" in BatchedFilter.group_mix.__doc__
    assert "group_mix_dev" in open(os.path.join(repo_root, "include", "fbus", "batched_filter.hpp")).read()


# ---- noise.imm_transition, noise.group_mix_weights ------------------------------------------------------------------------------------

def test_imm_transition_rows_sum_to_one():
    for G in (2, 3, 9, 64):
        for stay in (0.0, 0.5, 0.9, 0.95, 1.0):
            t = noise.imm_transition(G, stay)
            assert t.shape == (G, G) and t.dtype == np.float64 and (np.diag(t) == stay).all()
            assert np.abs(t.sum(axis=1) - 1.0).max() <= 1e-15 * G
            off = t[~np.eye(G, dtype=bool)]
            assert (off == off[0]).all() and abs(off[0] - (1.0 - stay) / (G - 1)) <= 1e-17
            assert noise.check_transition(t, G) is not None
    for bad in ((1, 0.5), (3, 1.5), (3, -0.1)):
        with pytest.raises(ValueError):
            noise.imm_transition(*bad)


def test_check_transition_names_the_row():
    t = noise.imm_transition(4, 0.9)
    for val, word in ((np.nan, "row 2"), (-0.1, "row 2"), (0.5, "row 2 sums")):
        bad = t.copy()
        bad[2, 1] = val
        with pytest.raises(ValueError) as e:
            noise.check_transition(bad, 4)
        assert word in str(e.value)
    with pytest.raises(ValueError):
        noise.check_transition(t, 3)


def test_group_mix_weights_follow_the_definition():
    rng = np.random.default_rng(1)
    for G in (2, 3, 9, 64):
        lw = rng.uniform(-4.0, 0.0, 5 * G) - 100.0
        lw[1], lw[G + 1], lw[2 * G] = -np.inf, np.nan, np.inf     # one excluded member in each of three groups
        mu, _ = noise.group_weights(lw, G)
        # the identity: W = I on the usable members, logc = log mu
        w, logc, W = noise.group_mix_weights(lw, np.eye(G), G)
        assert np.array_equal(w, mu) and W.shape == (5, G, G)
        ok = mu.reshape(5, G) > 0
        assert np.array_equal(W, np.eye(G)[None] * ok[:, None, :])
        with np.errstate(divide="ignore"):
            assert np.array_equal(logc, np.log(mu))
        assert (logc[[1, G + 1, 2 * G]] == -np.inf).all() and (mu[[1, G + 1, 2 * G]] == 0).all()
        # a sticky matrix: the columns of W sum to 1, the excluded sources have exact zeros, sum_j c_j = 1
        w, logc, W = noise.group_mix_weights(lw, noise.imm_transition(G, 0.95), G)
        assert np.isfinite(logc).all() and np.abs(W.sum(axis=1) - 1.0).max() <= 4e-16 * G
        assert (W[0, 1, :] == 0).all() and (W[1, 1, :] == 0).all() and (W[2, 0, :] == 0).all() and not np.isnan(W).any()
        assert np.abs(np.exp(logc).reshape(5, G).sum(axis=1) - 1.0).max() <= 4e-16 * G
        # the restatement of tests/group_mix_ref.py agrees group by group
        for g in range(5):
            mr, _, cr, Wr = group_mix_ref.mix_weights(lw[g * G:(g + 1) * G], noise.imm_transition(G, 0.95))
            assert np.array_equal(mr, w[g * G:(g + 1) * G]) and np.array_equal(Wr, W[g])
            assert np.array_equal(np.log(cr), logc[g * G:(g + 1) * G])
    # nobody usable, and a column of zeros
    w, logc, W = noise.group_mix_weights([np.nan, -np.inf, -1.0, -2.0], [[0.0, 1.0], [0.0, 1.0]], 2)
    assert not w[:2].any() and (logc[:2] == -np.inf).all() and not W[0].any()
    assert logc[2] == -np.inf and abs(logc[3]) <= 1e-15 and not W[1][:, 0].any() and np.array_equal(W[1][:, 1], w[2:])


# ---- tests/group_mix_ref.py on itself ---------------------------------------------------------------------------------------------------

def _group(rng, G, N):
    """G members about one sigma apart (the spread of tests/test_group_gpu.py), random SPD covariances, rot = anything recognisable"""
    sigma = np.repeat([1e-2, 2e-2, 1e-3, 5e-3, 1e-3, 5e-2], 3)
    base = np.zeros(19)
    base[0:3], base[3:6] = rng.normal(0, 1.0, 3), rng.normal(0, 0.1, 3)
    q = np.array([1.0, 0, 0, 0]) + rng.normal(0, 0.3, 4)
    base[6:10] = q / np.linalg.norm(q)
    base[10:16], base[16:19] = rng.normal(0, 0.01, 6), [0.1, -0.2, 9.8]
    nom = np.tile(base, (G, 1))
    off = rng.normal(0, 1.0, (G, 18)) * sigma
    nom[:, 0:3] += off[:, 0:3]
    nom[:, 3:6] += off[:, 3:6]
    nom[:, 10:16] += off[:, 9:15]
    if N == 18:
        nom[:, 16:19] += off[:, 15:18]
    for i in range(G):
        q = group_ref.qmul(nom[i, 6:10], group_ref.dq(off[i, 6:9]))
        nom[i, 6:10] = q / np.linalg.norm(q)
    A = rng.normal(0, 1.0, (G, N, N))
    P = (A @ np.swapaxes(A, 1, 2) / N + np.eye(N)) * (sigma[:N, None] * sigma[None, :N])
    P = 0.5 * (P + np.swapaxes(P, 1, 2))
    rot = rng.normal(0, 1.0, (G, 9))
    logw = rng.uniform(-4.0, 0.0, G) - 250.0
    return nom, rot, P, logw


def test_group_mix_ref_the_identity_changes_nothing():
    rng = np.random.default_rng(2)
    for G, N in ((2, 18), (5, 15), (9, 18)):
        nom, rot, P, logw = _group(rng, G, N)
        logw[0] = -np.inf
        if G > 2:
            logw[2], nom[2], P[2] = np.nan, np.nan, np.nan
        mu, logc, n2, r2, P2 = group_mix_ref.mix_group(nom, rot, P, logw, np.eye(G))
        for x, y in ((n2, nom), (r2, rot), (P2, P)):
            assert np.array_equal(x, y, equal_nan=True)
        with np.errstate(divide="ignore"):
            assert np.array_equal(logc, np.log(mu)) and logc[0] == -np.inf


def test_group_mix_ref_equal_rows_give_every_target_the_fused_estimate():
    """trans with every row equal to pi is the rank-one case: W_ij = mu_i for every target, so each target is group_fuse's estimate and
    c = pi.  Figures of this test as written: state 2.8e-17, covariance 5.2e-18, logc 4.4e-16; held to 1e-15, 1e-17, 1e-15."""
    rng = np.random.default_rng(3)
    worst = np.zeros(3)
    for G, N in ((2, 18), (3, 15), (8, 18), (32, 18)):
        nom, rot, P, logw = _group(rng, G, N)
        if G > 2:
            logw[1], nom[1], P[1] = np.nan, np.nan, np.nan         # an excluded NaN member is re-seeded like every other target
        pi = rng.uniform(0.5, 1.0, G)                              # (|log pi| < 4: one ulp of logc is 4.4e-16)
        pi /= pi.sum()
        mu, logc, n2, r2, P2 = group_mix_ref.mix_group(nom, rot, P, logw, np.tile(pi, (G, 1)))
        w, best, xf, Pf = group_ref.fuse_group(nom, P, logw)
        assert np.array_equal(mu, w)
        worst = np.maximum(worst, [np.abs(n2 - xf).max(), np.abs(P2 - Pf).max(), np.abs(logc - np.log(pi)).max()])
        assert np.array_equal(r2, np.tile(rot[best], (G, 1)))
    print(f"[group_mix] rank-one against fuse_group: state {worst[0]:.2e}  covariance {worst[1]:.2e}  logc {worst[2]:.2e}")
    assert worst[0] <= 1e-15 and worst[1] <= 1e-17 and worst[2] <= 1e-15


def test_group_mix_ref_a_sticky_matrix_gives_proper_covariances():
    rng = np.random.default_rng(4)
    for G, N in ((2, 18), (4, 15), (9, 18)):
        nom, rot, P, logw = _group(rng, G, N)
        mu, logc, n2, r2, P2 = group_mix_ref.mix_group(nom, rot, P, logw, noise.imm_transition(G, 0.95))
        assert abs(np.exp(logc).sum() - 1.0) <= 1e-15 and abs(mu.sum() - 1.0) <= 1e-15
        for j in range(G):
            assert np.array_equal(P2[j], P2[j].T) and np.linalg.eigvalsh(P2[j]).min() > 0
            assert abs(np.linalg.norm(n2[j, 6:10]) - 1.0) <= 1e-15
        assert not np.array_equal(n2, nom) and np.array_equal(r2, np.tile(rot[int(np.argmax(logw))], (G, 1)))
        # the batch form stacks the groups and reads get_state()'s tuple
        prev = np.arange(2 * G, dtype=np.int32)
        W, LC, N2, R2, PP = group_mix_ref.mix((np.concatenate([nom, nom]), np.concatenate([rot, rot]), np.concatenate([P, P]), prev),
                                              np.concatenate([logw, logw]), noise.imm_transition(G, 0.95), G)
        for k in (0, 1):
            s = slice(k * G, (k + 1) * G)
            assert np.array_equal(W[s], mu) and np.array_equal(LC[s], logc) and np.array_equal(N2[s], n2) and np.array_equal(PP[s], P2)
            assert np.array_equal(R2[s], r2)
