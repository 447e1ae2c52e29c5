"""CPU suite for the per-filter innovation log-likelihood sums (include/fbus_ekf.h, fbus_ekf_loglik_*; added under FBUS_ABI_VERSION 8
without a bump): the four symbols and their null-handle checks, fbus_ekf.noise.best on hand-made arrays, and the two determinant
identities the kernels take log det S from, restated in numpy against slogdet(H P H' + R)."""
import ctypes as C

import numpy as np
import pytest

from fbus_ekf import capi, noise

NEW = ["fbus_ekf_loglik_enable", "fbus_ekf_loglik_reset", "fbus_ekf_loglik_get", "fbus_ekf_loglik_get_dev"]


def test_the_four_symbols_are_declared_exported_and_refuse_a_null_handle():
    declared = capi.declared_symbols()
    lib = capi.load_library()
    for n in NEW:
        assert n in declared, n
        assert hasattr(lib, n), n
    assert capi.ABI_VERSION == 8 and lib.fbus_ekf_abi_version() == 8
    assert lib.fbus_ekf_loglik_enable(None, 1) == 1
    assert lib.fbus_ekf_loglik_enable(None, 0) == 1
    assert lib.fbus_ekf_loglik_reset(None) == 1
    ll = (C.c_double * 4)()
    rows = (C.c_int64 * 4)()
    cnt = (C.c_int32 * 4)()
    for fn in ("fbus_ekf_loglik_get", "fbus_ekf_loglik_get_dev"):
        assert getattr(lib, fn)(None, ll, rows, cnt, cnt) == 1
        assert getattr(lib, fn)(None, None, None, None, None) == 1


def test_the_python_and_cxx_layers_carry_the_methods(repo_root):
    from fbus_ekf import BatchedFilter, replay
    import inspect
    import os
    for m in ("loglik_enable", "loglik_reset", "loglik"):
        assert callable(getattr(BatchedFilter, m))
    assert "loglik" in inspect.signature(replay.replay_windowed).parameters
    assert "loglik" in inspect.signature(replay.replay).parameters
    hdr = open(os.path.join(repo_root, "include", "fbus", "batched_filter.hpp")).read()
    for m in ("loglik_enable", "loglik_reset", "loglik()"):
        assert m in hdr, m


def test_best_sums_per_hypothesis_and_takes_the_first_arg_max():
    # uneven group sizes
    ll = np.array([-1.0, -2.0, -3.0, -0.5, -0.25, -10.0])
    hyp = np.array([0, 1, 0, 2, 2, 1])
    g, tot = noise.best(ll, hyp, 3)
    assert g == 2 and np.array_equal(tot, [-4.0, -12.0, -0.75])
    # a tie: the first of the equal totals
    g, tot = noise.best([-1.0, -1.0, -2.0, 0.0], [1, 0, 2, 2], 3)
    assert g == 0 and np.array_equal(tot, [-1.0, -1.0, -2.0])
    # a hypothesis no filter runs cannot win, even against negative totals
    g, tot = noise.best([-5.0, -7.0], [0, 2], 4)
    assert g == 0 and tot[1] == -np.inf and tot[3] == -np.inf and tot[2] == -7.0
    # the round-robin assignment of noise.grid
    prm = capi.default_params(0)
    table, hyp, rows = noise.grid(prm, 10, r_pix=[0.5, 1.0, 2.0])
    g, tot = noise.best(-(np.arange(10.0) + 1.0), hyp, len(rows))
    assert np.array_equal(tot, [-(1 + 4 + 7 + 10), -(2 + 5 + 8), -(3 + 6 + 9)]) and g == 1
    with pytest.raises(ValueError):
        noise.best([0.0, 1.0], [0, 3], 3)
    with pytest.raises(ValueError):
        noise.best([0.0, 1.0], [0], 3)


def _rand_spd(rng, n, scale):
    A = rng.normal(size=(n, n))
    return scale * (A @ A.T + 0.1 * np.eye(n))


def _chol_drop(A, rel=4e-15):
    """Cholesky with a pivot that is not clearly positive relative to its original diagonal dropped (info_solve's rule)"""
    n = len(A)
    A = A.copy()
    L = np.zeros((n, n))
    d0 = np.diag(A).copy()
    for a in range(n):
        piv = A[a, a]
        s = 1.0 / np.sqrt(piv) if piv > rel * d0[a] else 0.0
        L[a:, a] = A[a:, a] * s
        A[a + 1:, a + 1:] -= np.outer(L[a + 1:, a], L[a + 1:, a])
    return L


@pytest.mark.parametrize("case", ["pixels", "edge_on", "pose", "pose_zero_direction"])
def test_the_kernels_determinant_identities_equal_slogdet_S(case):
    """Sylvester: det S = det R det(I + P_JJ Lam), Lam = H_J' R^-1 H_J.
    pixel / corner rows (info_solve): Lam = Lc Lc', Mt = I + Lc' P_JJ Lc = Cm Cm', iC[a] = 1 / Cm(a, a):
        log det(I + P_JJ Lam) = -2 ln prod iC[a]        -- also with a dropped pivot of Lam (a marker seen edge-on)
    pose rows (pose_nis): P_JJ = C C', K = I + C' Lam C = D D':
        log det(I + P_JJ Lam) = ln prod D(a, a)^2       -- also with a zero direction of P_JJ (its pivot dropped: a factor 1)"""
    rng = np.random.default_rng({"pixels": 1, "edge_on": 2, "pose": 3, "pose_zero_direction": 4}[case])
    N, J = 18, [0, 1, 2, 6, 7, 8]
    for _ in range(20):
        pose = case.startswith("pose")
        P = _rand_spd(rng, N, 1e-4 if pose else 1e-7)
        m = 28 if pose else 32
        H = np.zeros((m, N))
        H[:, J] = rng.normal(size=(m, 6)) * (1.0 if pose else 300.0)
        if case == "edge_on":
            H[:, J[5]] = 0.0                                  # no row sees the last direction: Lam has one zero pivot
        if case == "pose_zero_direction":
            P[J[2], :] = 0.0; P[:, J[2]] = 0.0                # no prior uncertainty along z
        Rd = np.tile([1e-4] * 3 + [4e-4] * 4, 4) if pose else np.full(m, 0.37)
        S = H @ P @ H.T + np.diag(Rd)
        sign, ref = np.linalg.slogdet(S)
        assert sign > 0
        HJ, PJJ = H[:, J], P[np.ix_(J, J)]
        Lam = HJ.T @ (HJ / Rd[:, None])
        lndetR = float(np.sum(np.log(Rd)))
        if pose:
            Cf = _chol_drop(PJJ, 0.0)
            D = np.linalg.cholesky(np.eye(6) + Cf.T @ Lam @ Cf)
            got = lndetR + np.log(np.prod(np.diag(D) ** 2))
            if case == "pose_zero_direction":
                assert Cf[2, 2] == 0.0 and abs(D[2, 2] - 1.0) < 1e-12
        else:
            Lc = _chol_drop(Lam)
            if case == "edge_on":
                assert np.all(Lc[:, 5] == 0.0)
            Cm = np.linalg.cholesky(np.eye(6) + Lc.T @ PJJ @ Lc)
            icp = np.prod(1.0 / np.diag(Cm))
            got = lndetR + np.log(1.0 / (icp * icp))
        assert abs(got - ref) <= 1e-9 * max(abs(ref), 1.0), (case, got, ref)
        # the gate of the GPU test is sharp enough for these: a missing factor 2 on the Cholesky logarithms, one row's ln r left out
        assert abs(0.5 * (got - lndetR)) > 10 * 1e-4 and abs(np.log(Rd[0])) > 10 * 1e-4
