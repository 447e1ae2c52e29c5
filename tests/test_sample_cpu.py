"""fbus_ekf_sample without a GPU: the numpy restatement (tests/sample_ref.py) closed against tests/nees_ref.py, the sigma points of
fbus_ekf.consistency, the chi-square calibration of drawn states, and the two symbols.

Bounds.  The round trip and the sigma-point moments are identities of exact arithmetic.  In float64 a drawn row is a state rounded to
double: a component of size < 16 (g is 9.81) carries an error of up to 2^-53 x 16 = 1.8e-15, and the error state read back from it is known
no better.  Relative to an error component -- sigma is 1e-3 .. 1e-1 here, and of a few thousand normal draws none is expected below 1e-4
sigma -- that is some 1e-15 / 1e-7 = 1e-8 at the very worst and typically 1e-13 .. 1e-11; the sums of squares, dominated by their large
terms, sit near 1e-14.  The bound is 1e-10, the one tests/test_nees_cpu.py gives the gap of the two paths of its reference; the figures
are printed.  The calibration bounds are those of tests/test_nees_cpu.py: derived from the chi-square law, 5 sigma."""
import ctypes as C
import math

import numpy as np
import pytest

import nees_ref
import sample_ref
from fbus_ekf import capi, consistency, gating

N_CAL = 8192


@pytest.fixture(scope="module")
def cal():
    nom, rot, P, prev, _ = nees_ref.calibration_inputs(N_CAL, 18, 1)
    xi = np.random.default_rng(11).normal(size=(1, N_CAL, 18))
    for a in (nom, P, xi):
        a.setflags(write=False)
    return nom, P, xi


def calibrated(col, dof, n):
    mean, share = float(col.mean()), float((col > gating.chi2_ppf(0.95, dof)).mean())
    bm, bs = 5 * math.sqrt(2 * dof / n), 5 * math.sqrt(0.05 * 0.95 / n)
    print(f"dof {dof}: mean {mean:.3f} against {dof} +- {bm:.3f}, share {share:.4f} against 0.05 +- {bs:.4f}")
    return abs(mean - dof) <= bm and abs(share - 0.05) <= bs


# ---- 1. the round trip of the reference -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nstate", [18, 15])
def test_a_drawn_row_fed_back_as_truth_returns_the_prefix_sums_of_xi_squared(cal, nstate):
    nom, P, xi = cal
    n = 512
    nom, P = nom[:n], P[:n, :nstate, :nstate]
    xi = np.random.default_rng(12).normal(size=(2, n, nstate))
    rows, drawn, d = sample_ref.sample(nom, P, xi)
    assert drawn.all() and np.isfinite(rows).all()
    cols, err = sample_ref.loop(nom, P, xi, rows)
    full, pose, p = sample_ref.prefix_sums(xi)
    gaps = [nees_ref.rel_gap(cols[:, :, c], want) for c, want in enumerate((full, pose, p))]
    gaps.append(nees_ref.rel_gap(err, sample_ref.delta(P, xi, np.longdouble)[0]))
    print(f"N={nstate}: FULL {gaps[0]:.2e} POSE {gaps[1]:.2e} P {gaps[2]:.2e} err {gaps[3]:.2e}, cond(P) <= {np.linalg.cond(P).max():.0f}")
    assert max(gaps) < 1e-10
    # the quaternion of every row is a unit quaternion, and g of an N = 15 filter is the record's
    assert np.abs(np.linalg.norm(rows[:, :, 6:10], axis=2) - 1).max() < 4e-16
    if nstate == 15:
        assert np.array_equal(rows[:, :, 16:19], np.broadcast_to(nom[:, 16:19], (2, n, 3)))
    # and the longdouble path agrees
    rl = sample_ref.sample(nom, P, xi, dtype=np.longdouble)[0]
    assert np.abs(rows - rl).max() < 1e-14


def test_exits_of_the_reference(cal):
    nom, P, xi = cal
    nom, P = nom[:6].copy(), P[:6].copy()
    xi = np.array(xi[:, :6])
    P[1, 3, 7] = P[1, 7, 3] = np.nan
    P[2, 1, 1] = -P[2, 1, 1]
    nom[2, 4] = -0.0
    xi[0, 4] = np.nan
    skip = np.zeros(6, np.uint8); skip[3] = 1
    rows, drawn, _ = sample_ref.sample(nom, P, xi, skip)
    assert list(drawn) == [1, 0, 0, 0, 1, 1]
    for b in (1, 2, 3):
        assert np.array_equal(rows[0, b].view(np.uint64), nom[b].view(np.uint64))
    assert not np.isfinite(rows[0, 4]).any() and np.isfinite(rows[0, [0, 5]]).all()


# ---- 2. sigma points --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nstate,kappa", [(18, 0.0), (15, 0.0), (18, 1.5)])
def test_sigma_points_carry_the_mean_and_the_covariance(cal, nstate, kappa):
    nom, P, _ = cal
    n = 256
    nom, P = nom[:n], P[:n, :nstate, :nstate]
    xi, w = consistency.sigma_points(nstate, kappa)
    assert xi.shape == (2 * nstate + 1, nstate) and w.shape == (2 * nstate + 1,)
    assert not xi[0].any() and w[0] == pytest.approx(kappa / (nstate + kappa), abs=1e-16)
    assert abs(w.sum() - 1) < 1e-15
    assert np.abs(np.einsum("s,si->i", w, xi)).max() == 0
    assert np.abs(np.einsum("s,si,sj->ij", w, xi, xi) - np.eye(nstate)).max() < 1e-14
    rows, drawn, _ = sample_ref.sample(nom, P, np.broadcast_to(xi[:, None, :], (len(xi), n, nstate)))
    assert drawn.all()
    gm, gc = sample_ref.moment_gaps(nom, P, rows, w)
    print(f"N={nstate} kappa={kappa}: |sum w delta| / sigma {gm:.2e}, |sum w delta delta' - P| / sqrt(P_ii P_jj) {gc:.2e}")
    assert gm < 1e-10 and gc < 1e-10
    with pytest.raises(ValueError):
        consistency.sigma_points(12)
    with pytest.raises(ValueError):
        consistency.sigma_points(18, -18.0)


# ---- 3. calibration -----------------------------------------------------------------------------------------------------------------------
def test_states_drawn_by_the_reference_are_calibrated_in_every_column(cal):
    nom, P, xi = cal
    rows, drawn, _ = sample_ref.sample(nom, P, xi)
    assert drawn.all()
    nees = nees_ref.nees(nom, P, rows[0])[0]
    assert np.isfinite(nees).all()
    ok = [calibrated(nees[:, c], dof, N_CAL) for c, dof in enumerate(consistency.nees_dof(18))]
    assert all(ok), ok


# ---- 4. the symbols -----------------------------------------------------------------------------------------------------------------------
def test_the_two_symbols_are_declared_exported_prototyped_and_refuse_a_null_handle():
    declared = capi.declared_symbols()
    lib = capi.load_library()
    xi = (C.c_double * 18)()
    out = (C.c_double * 19)()
    drawn = (C.c_uint8 * 1)()
    for n in ("fbus_ekf_sample", "fbus_ekf_sample_dev"):
        assert n in declared, n
        assert hasattr(lib, n), n
        assert getattr(lib, n).argtypes is not None and len(getattr(lib, n).argtypes) == 6, n
        assert getattr(lib, n)(None, 1, xi, None, out, drawn) == 1
        assert getattr(lib, n)(None, 0, None, None, None, None) == 1
    assert capi.ABI_VERSION == 8 and lib.fbus_ekf_abi_version() == 8
    assert capi.SAMPLE_MAX == 256
