"""CPU suite for the NIS output and chi-square gating of the pixel / corner updates (include/fbus_ekf.h, FBUS_ABI_VERSION 8):
the new symbols and their null-handle checks, fbus_ekf.gating.chi2_gate against scipy (or its own defining series), and the two
identities the kernels evaluate the NIS by, restated in numpy against r' (H P H' + R)^-1 r."""
import ctypes as C
import math

import numpy as np
import pytest

from fbus_ekf import capi, gating

NEW = ["fbus_ekf_set_gate", "fbus_ekf_correct_nis", "fbus_ekf_correct_nis_dev", "fbus_ekf_correct_pixels_nis", "fbus_ekf_correct_pixels_nis_dev",
       "fbus_ekf_correct_corners_nis", "fbus_ekf_correct_corners_nis_dev"]


def test_new_symbols_are_declared_exported_and_refuse_a_null_handle():
    declared = capi.declared_symbols()
    lib = capi.load_library()
    for n in NEW:
        assert n in declared, n
        assert hasattr(lib, n), n
    assert capi.ABI_VERSION == 8 and lib.fbus_ekf_abi_version() == 8
    assert capi.GATE_MAX_DOF == 256
    thr = (C.c_double * 3)(math.inf, 1.0, 2.0)
    assert lib.fbus_ekf_set_gate(None, 3, thr) == 1
    assert lib.fbus_ekf_set_gate(None, 0, None) == 1
    ids = (C.c_int32 * 4)()
    buf = (C.c_float * 64)()
    for fn in ("fbus_ekf_correct_nis", "fbus_ekf_correct_nis_dev"):
        assert getattr(lib, fn)(None, 4, ids, buf, buf, capi.MODE_STACKED, None, None, None) == 1
    for fn in ("fbus_ekf_correct_pixels_nis", "fbus_ekf_correct_pixels_nis_dev"):
        assert getattr(lib, fn)(None, 4, ids, buf, None, None, None, None) == 1
    for fn in ("fbus_ekf_correct_corners_nis", "fbus_ekf_correct_corners_nis_dev"):
        assert getattr(lib, fn)(None, 4, ids, buf, buf, capi.VIS_REFRACTIVE, capi.MODE_STACKED, None, None, None) == 1


def _gammp_series(a, x):
    # P(a, x) = x^a e^-x / Gamma(a + 1) * sum_n x^n / ((a + 1) ... (a + n)), summed in log space term by term
    s, term, n = 1.0, 1.0, 0
    while True:
        n += 1
        term *= x / (a + n)
        s += term
        if term < 1e-18 * s:
            break
    return math.exp(a * math.log(x) - x - math.lgamma(a + 1.0)) * s


@pytest.mark.parametrize("prob", [0.9, 0.99, 0.999])
def test_chi2_gate_is_the_chi_square_quantile(prob):
    thr = gating.chi2_gate(prob)
    assert thr.shape == (capi.GATE_MAX_DOF + 1,) and thr[0] == math.inf
    d = np.arange(1, capi.GATE_MAX_DOF + 1)
    try:
        from scipy.stats import chi2
    except ImportError:
        chi2 = None
    if chi2 is not None:
        ref = chi2.ppf(prob, d)
        np.testing.assert_allclose(thr[1:], ref, rtol=1e-9, atol=0)
    for k in d:                                           # the defining equation, independent of scipy: P(d / 2, thr / 2) = prob
        assert abs(_gammp_series(0.5 * k, 0.5 * thr[k]) - prob) < 1e-10, k
    assert len(gating.chi2_gate(prob, 10)) == 11


def _rand_spd(rng, n, scale):
    A = rng.normal(size=(n, n))
    return scale * (A @ A.T + 0.1 * np.eye(n))


@pytest.mark.parametrize("case", ["pixels", "pose", "collinear"])
def test_the_kernels_identities_equal_r_S_inverse_r(case):
    """pixel / corner rows: NIS = w sum res^2 - b' P_JJ G' b (G = (I + P_JJ Lam)^-1, the kernels' m = G' b);
    pose rows: NIS = sum w res^2 - b' (P_JJ^-1 + Lam)^-1 b.  Both equal r' (H P H' + R)^-1 r, also for a rank-deficient Lam
    (one marker whose corners are collinear: H_J has rank < 6)."""
    rng = np.random.default_rng({"pixels": 1, "pose": 2, "collinear": 3}[case])
    N, J = 18, [0, 1, 2, 6, 7, 8]
    for _ in range(20):
        P = _rand_spd(rng, N, 1e-7 if case != "pose" else 1e-4)     # |P_JJ Lam| of order 10-100, as after a few updates
        nrow = 32 if case != "collinear" else 12
        Hj = rng.normal(size=(nrow, 6))
        if case == "collinear":                           # 4 corners on a line: rows from 2 independent points only
            Hj[6:] = Hj[:6] * rng.normal(size=(6, 1))
            Hj[:, 5] = 0.0
        H = np.zeros((nrow, N))
        H[:, J] = Hj
        w = 1.0 / 1e-6 if case != "pose" else None
        rdiag = np.full(nrow, 1e-6) if case != "pose" else rng.uniform(1e-4, 1e-2, nrow)
        r = rng.normal(size=nrow) * np.sqrt(rdiag) * 3
        S = H @ P @ H.T + np.diag(rdiag)
        ref = r @ np.linalg.solve(S, r)
        Lam = Hj.T @ (Hj / rdiag[:, None])
        b = Hj.T @ (r / rdiag)
        PJJ = P[np.ix_(J, J)]
        if case == "pose":
            nis = np.sum(r * r / rdiag) - b @ np.linalg.solve(np.linalg.inv(PJJ) + Lam, b)
            # the form the kernels solve: (I + P_JJ Lam) y = P_JJ b, nis = sum w res^2 - b' y
            y = np.linalg.solve(np.eye(6) + PJJ @ Lam, PJJ @ b)
            nis2 = np.sum(r * r / rdiag) - b @ y
        else:
            m = np.linalg.solve((np.eye(6) + PJJ @ Lam).T, b)          # m = G' b
            nis = w * np.sum(r * r) - b @ PJJ @ m
            nis2 = nis
        assert abs(nis - ref) <= 1e-12 * max(ref, 1.0) * max(1.0, np.sum(r * r / rdiag) / ref), (nis, ref)
        assert abs(nis2 - ref) <= 1e-12 * max(ref, 1.0) * max(1.0, np.sum(r * r / rdiag) / ref), (nis2, ref)
