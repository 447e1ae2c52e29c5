"""CPU suite for the hypothesis groups (include/fbus_ekf.h, fbus_ekf_group_fuse / fbus_ekf_group_collapse; added under
FBUS_ABI_VERSION 8 without a bump): the four symbols and their null-handle checks, fbus_ekf.noise.group_weights on hand-made arrays,
and tests/group_ref.py -- the fp64 restatement the GPU suite holds the kernels to -- on cases whose answer is known in closed form."""
import ctypes as C
import os

import numpy as np

import group_ref
from fbus_ekf import capi, noise

NEW = ["fbus_ekf_group_fuse", "fbus_ekf_group_fuse_dev", "fbus_ekf_group_collapse", "fbus_ekf_group_collapse_dev"]


def test_the_four_symbols_are_declared_exported_and_refuse_a_null_handle():
    declared = capi.declared_symbols()
    lib = capi.load_library()
    for n in NEW:
        assert n in declared, n
        assert hasattr(lib, n), n
    assert capi.ABI_VERSION == 8 and lib.fbus_ekf_abi_version() == 8 and capi.GROUP_MAX == 64
    w = (C.c_double * 4)()
    best = (C.c_int32 * 2)()
    for fn in ("fbus_ekf_group_fuse", "fbus_ekf_group_fuse_dev"):
        assert getattr(lib, fn)(None, 2, w, w, best, None, None, None) == 1
        assert getattr(lib, fn)(None, 2, None, None, None, None, None, None) == 1
    for fn in ("fbus_ekf_group_collapse", "fbus_ekf_group_collapse_dev"):
        assert getattr(lib, fn)(None, 2, best) == 1
        assert getattr(lib, fn)(None, 2, None) == 1


def test_the_python_and_cxx_layers_carry_the_methods(repo_root):
    from fbus_ekf import BatchedFilter
    for m in ("group_fuse", "group_collapse"):
        assert callable(getattr(BatchedFilter, m))
    hdr = open(os.path.join(repo_root, "include", "fbus", "batched_filter.hpp")).read()
    for m in ("group_fuse_dev", "group_collapse_dev"):
        assert m in hdr, m
    assert "#define FBUS_GROUP_MAX 64" in open(os.path.join(repo_root, "include", "fbus_ekf.h")).read()


# ---- noise.group_weights --------------------------------------------------------------------------------------------------------------

def test_group_weights_sum_to_one_and_follow_the_definition():
    rng = np.random.default_rng(1)
    for G in (2, 3, 9, 64):
        lw = rng.uniform(-4.0, 0.0, 5 * G)
        w, best = noise.group_weights(lw, G)
        assert w.shape == (5 * G,) and best.shape == (5,) and w.dtype == np.float64 and best.dtype == np.int32
        assert np.abs(w.reshape(5, G).sum(axis=1) - 1.0).max() < 1e-15 * G
        e = np.exp(lw.reshape(5, G) - lw.reshape(5, G).max(axis=1, keepdims=True))
        assert np.abs(w.reshape(5, G) - e / e.sum(axis=1, keepdims=True)).max() < 1e-15
        assert np.array_equal(best, lw.reshape(5, G).argmax(axis=1))
        # the restatement of tests/group_ref.py agrees group by group
        for j in range(5):
            wr, br = group_ref.weights(lw[j * G:(j + 1) * G])
            assert br == best[j] and np.abs(wr - w[j * G:(j + 1) * G]).max() < 1e-15


def test_group_weights_exclude_non_finite_entries():
    lw = np.array([-1.0, -np.inf, -2.0, np.nan,         # -inf and NaN are excluded
                   np.inf, -3.0, -3.0, -4.0,            # +inf is excluded too: it does not win
                   np.nan, np.inf, -np.inf, np.nan])    # nobody usable
    w, best = noise.group_weights(lw, 4)
    e = np.exp([-1.0 + 1.0, -2.0 + 1.0])
    assert w[1] == 0.0 and w[3] == 0.0 and np.allclose(w[[0, 2]], e / e.sum(), rtol=0, atol=1e-16) and best[0] == 0
    assert w[4] == 0.0 and best[1] == 1 and abs(w[4:8].sum() - 1.0) < 1e-15 and w[5] == w[6]      # the tie goes to the first member
    assert np.array_equal(w[8:12], np.zeros(4)) and best[2] == -1
    assert not np.isnan(w).any()


def test_group_weights_neither_overflow_nor_collapse_far_from_zero():
    lw = -1.0e6 + np.array([0.0, -0.5, -1.0, 0.25])
    w, best = noise.group_weights(lw, 4)
    e = np.exp(np.array([0.0, -0.5, -1.0, 0.25]) - 0.25)
    assert best[0] == 3 and np.isfinite(w).all() and (w > 0.05).all()
    assert np.abs(w - e / e.sum()).max() < 1e-15
    w, best = noise.group_weights(-lw, 4)                   # and around +1e6
    assert best[0] == 2 and np.isfinite(w).all() and abs(w.sum() - 1.0) < 1e-15


def test_group_weights_ties_go_to_the_first_member():
    w, best = noise.group_weights([-2.0, -1.0, -1.0, -7.0, -7.0, -1.0, 3.0, 3.0, 3.0], 3)
    assert np.array_equal(best, [1, 2, 0])
    assert np.abs(w[:3] - np.array([np.exp(-1.0), 1.0, 1.0]) / (np.exp(-1.0) + 2.0)).max() < 1e-15 and w[1] == w[2]
    assert np.abs(w[3:6] - np.array([np.exp(-6.0), np.exp(-6.0), 1.0]) / (2.0 * np.exp(-6.0) + 1.0)).max() < 1e-15
    assert np.abs(w[6:] - 1.0 / 3.0).max() < 1e-16


# ---- tests/group_ref.py on itself -----------------------------------------------------------------------------------------------------

def _member(rng, N):
    nom = np.zeros(19)
    nom[0:3] = rng.normal(0, 1.0, 3)
    nom[3:6] = rng.normal(0, 0.1, 3)
    q = np.array([1.0, 0, 0, 0]) + rng.normal(0, 0.3, 4)
    nom[6:10] = q / np.linalg.norm(q)
    nom[10:16] = rng.normal(0, 0.01, 6)
    nom[16:19] = [9.8, 0.0, 0.0]
    A = rng.normal(0, 1.0, (N, N))
    return nom, 1e-4 * (A @ A.T / N + np.eye(N))


def test_group_ref_identical_members_give_that_member():
    rng = np.random.default_rng(2)
    for N in (18, 15):
        nom, P = _member(rng, N)
        w, best, x, Pb = group_ref.fuse_group(np.tile(nom, (5, 1)), np.tile(P, (5, 1, 1)), [-1.0, -3.0, -0.5, -0.5, -2.0])
        assert best == 2 and abs(w.sum() - 1.0) < 1e-15
        assert np.abs(x - nom).max() < 1e-15 and np.abs(Pb - P).max() < 1e-18


def test_group_ref_one_hot_weights_give_the_best_member():
    rng = np.random.default_rng(3)
    mem = [_member(rng, 18) for _ in range(4)]
    nom, P = np.array([m[0] for m in mem]), np.array([m[1] for m in mem])
    for lw, k in (([-np.inf, np.nan, -5.0, np.inf], 2), ([-2000.0, 0.0, -1500.0, -900.0], 1)):      # excluded, and underflowed to 0
        w, best, x, Pb = group_ref.fuse_group(nom, P, lw)
        assert best == k and w[k] == 1.0 and w.sum() == 1.0
        assert np.abs(x - nom[k]).max() < 1e-15 and np.array_equal(Pb, P[k])
    # a NaN record behind a zero weight changes nothing
    nom2, P2 = nom.copy(), P.copy()
    nom2[0], P2[0] = np.nan, np.nan
    w, best, x, Pb = group_ref.fuse_group(nom2, P2, [np.nan, -1.0, -1.5, -np.inf])
    w3, best3, x3, Pb3 = group_ref.fuse_group(nom[1:3], P[1:3], [-1.0, -1.5])
    assert best == 1 and best3 == 0 and np.isfinite(x).all() and np.isfinite(Pb).all()
    assert np.array_equal(w[1:3], w3) and np.array_equal(x, x3) and np.array_equal(Pb, Pb3)
    # nobody usable: member 0, copied
    w, best, x, Pb = group_ref.fuse_group(nom, P, [np.nan, np.inf, -np.inf, np.nan])
    assert best == -1 and not w.any() and np.array_equal(x, nom[0]) and np.array_equal(Pb, P[0])


def test_group_ref_two_members_match_the_closed_form():
    """two members that differ by dp in the position and by a rotation theta about z, weights (w0, w1) with member 0 the best:
    mu = w1 delta, the fused state is x0 (+) w1 delta, and the spread adds w0 w1 delta delta' to the weighted mean of the covariances"""
    rng = np.random.default_rng(4)
    nom0, P0 = _member(rng, 18)
    _, P1 = _member(rng, 18)
    dp, th = np.array([0.02, -0.01, 0.03]), 0.004
    nom1 = nom0.copy()
    nom1[0:3] += dp
    nom1[6:10] = group_ref.qmul(nom0[6:10], group_ref.dq(np.array([0.0, 0.0, th])))
    lw = np.array([np.log(0.7), np.log(0.3)]) - 12.0
    w, best, x, Pb = group_ref.fuse_group(np.array([nom0, nom1]), np.array([P0, P1]), lw)
    assert best == 0 and np.abs(w - [0.7, 0.3]).max() < 1e-15
    delta = np.zeros(18)
    delta[0:3], delta[8] = dp, th
    assert np.abs(group_ref.delta(nom1, nom0, 18) - delta).max() < 1e-15
    assert np.abs(x[0:3] - (nom0[0:3] + 0.3 * dp)).max() < 1e-15
    qf = group_ref.qmul(nom0[6:10], group_ref.dq(np.array([0.0, 0.0, 0.3 * th])))
    assert np.abs(x[6:10] - qf).max() < 1e-15
    assert np.array_equal(x[3:6], nom0[3:6]) and np.array_equal(x[10:19], nom0[10:19])
    want = 0.7 * P0 + 0.3 * P1 + 0.7 * 0.3 * np.outer(delta, delta)
    assert np.abs(Pb - want).max() < 1e-17 and np.array_equal(Pb, Pb.T)
    # the batch form stacks the groups
    W, Bst, X, PB = group_ref.fuse(np.array([nom0, nom1, nom1, nom0]), np.array([P0, P1, P1, P0]), np.concatenate([lw, lw[::-1]]), 2)
    assert np.array_equal(Bst, [0, 1]) and np.array_equal(W[:2], w) and np.array_equal(X[0], x) and np.array_equal(PB[0], Pb)
    assert np.abs(X[1] - x).max() < 1e-15 and np.abs(PB[1] - Pb).max() < 1e-17
