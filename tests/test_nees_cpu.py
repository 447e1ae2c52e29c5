"""fbus_ekf_nees without a GPU: the numpy restatement against itself and against np.linalg, the calibration of the inputs the device test
uses, fbus_ekf.consistency, and the two symbols.  The bounds of the calibration are derived, not measured: under truth ~ N(estimate, P) a
column is chi-square with dof degrees of freedom (mean dof, variance 2 dof), so the mean of n values lies within 5 sqrt(2 dof / n) of dof,
and the share above the 95 % quantile within 5 sqrt(0.05 x 0.95 / n) of 0.05, each but for a 5-sigma event (6e-7)."""
import ctypes as C
import math

import numpy as np
import pytest

import nees_ref
from fbus_ekf import capi, consistency, gating

N_CAL = 8192


@pytest.fixture(scope="module")
def cal():
    nom, rot, P, prev, truth = nees_ref.calibration_inputs(N_CAL, 18, 1)
    out = nees_ref.nees(nom, P, truth)
    for a in (nom, P, truth) + out:
        a.setflags(write=False)
    return nom, P, truth, out


def calibrated(col, dof, n):
    """(mean, share above the 95 % quantile, and whether both meet the derived bounds); prints the figures"""
    mean, share = float(col.mean()), float((col > gating.chi2_ppf(0.95, dof)).mean())
    bm, bs = 5 * math.sqrt(2 * dof / n), 5 * math.sqrt(0.05 * 0.95 / n)
    print(f"dof {dof}: mean {mean:.3f} against {dof} +- {bm:.3f}, share {share:.4f} against 0.05 +- {bs:.4f}")
    return mean, share, abs(mean - dof) <= bm and abs(share - 0.05) <= bs


# ---- 1. the reference against itself ---------------------------------------------------------------------------------------------------
def test_full_equals_numpy_solve_and_lnp_numpy_slogdet(cal):
    nom, P, truth, (nees, err, lnp) = cal
    sel = slice(0, 256)
    ref = np.einsum("bi,bi->b", err[sel], np.linalg.solve(P[sel], err[sel][..., None])[..., 0])
    np.testing.assert_allclose(nees[sel, 0], ref, rtol=1e-9)
    sign, logdet = np.linalg.slogdet(P[sel])
    assert (sign > 0).all()
    np.testing.assert_allclose(lnp[sel], -0.5 * (ref + logdet + 18 * math.log(2 * math.pi)), rtol=1e-9)


def test_a_block_column_equals_the_reference_on_that_marginal_alone(cal):
    nom, P, truth, (nees, err, lnp) = cal
    sel = slice(0, 256)
    for c, Jc in enumerate(nees_ref.blocks(18)):
        A, d = P[sel][:, Jc][:, :, Jc], err[sel][:, Jc]
        assert np.array_equal(nees[sel, c], nees_ref.block_nees(A, d)), c
        np.testing.assert_allclose(nees[sel, c], np.einsum("bi,bi->b", d, np.linalg.solve(A, d[..., None])[..., 0]), rtol=1e-9)


def test_the_leading_entries_of_the_solve_depend_on_the_leading_block_only(cal):
    """factorised in the order p, theta, v, ba, bg, g, the prefix sums of |L^-1 delta|^2 are the P, POSE and FULL columns"""
    nom, P, truth, (nees, err, lnp) = cal
    sel = slice(0, 256)
    order = [0, 1, 2, 6, 7, 8, 3, 4, 5] + list(range(9, 18))
    y, piv, bad = nees_ref.chol_solve(P[sel][:, order][:, :, order], err[sel][:, order])
    assert not bad.any()
    cs = np.cumsum(y * y, axis=1)
    np.testing.assert_allclose(cs[:, 2], nees[sel, capi.NEES_P], rtol=1e-12)
    np.testing.assert_allclose(cs[:, 5], nees[sel, capi.NEES_POSE], rtol=1e-12)
    np.testing.assert_allclose(cs[:, 17], nees[sel, capi.NEES_FULL], rtol=1e-10)
    # and bit for bit: the leading k entries are those of the k x k block factorised alone
    y6, _, _ = nees_ref.chol_solve(P[sel][:, order[:6]][:, :, order[:6]], err[sel][:, order[:6]])
    assert np.array_equal(y[:, :6], y6)


def test_nan_and_skip_rules_of_the_reference(cal):
    nom, P, truth, _ = cal
    nom, P, truth = nom[:8].copy(), P[:8].copy(), truth[:8].copy()
    nom[1, 13] = np.nan                     # bg of the record
    P[2, 4, 4] = -P[2, 4, 4]                # v
    truth[3, 6:10] = 0.0
    truth[4] = np.nan
    nom[5, 0] = np.nan                      # p of the record
    skip = np.zeros(8, np.uint8); skip[6] = 1
    nees, err, lnp = nees_ref.nees(nom, P, truth, skip)
    nanc = lambda b: set(np.nonzero(np.isnan(nees[b]))[0])
    assert nanc(0) == set() and np.isfinite(lnp[0])
    assert nanc(1) == {capi.NEES_FULL, capi.NEES_BG} and np.isnan(lnp[1])
    assert nanc(2) == {capi.NEES_FULL, capi.NEES_V}
    assert nanc(3) == {capi.NEES_FULL, capi.NEES_POSE, capi.NEES_THETA} and np.isnan(err[3, 6:9]).all() and np.isfinite(err[3, :6]).all()
    assert nanc(4) == set(range(8))
    assert nanc(5) == {capi.NEES_FULL, capi.NEES_POSE, capi.NEES_P}
    assert not nees[6].any() and not err[6].any() and lnp[6] == 0
    n15 = nees_ref.nees(nom, P[:, :15, :15], truth)[0]
    assert (n15[:, capi.NEES_G] == 0).all()


def test_the_longdouble_path_agrees_and_the_gap_is_small(cal):
    nom, P, truth, _ = cal
    gap = nees_ref.path_gap(nom[:512], P[:512], truth[:512])
    print(f"largest relative gap float64 / longdouble: {gap:.2e}")
    assert gap < 1e-10


# ---- 2. calibration of the inputs the device test uses ---------------------------------------------------------------------------------
def test_the_inputs_are_calibrated_in_every_column(cal):
    nees = cal[3][0]
    assert np.isfinite(nees).all()
    ok = [calibrated(nees[:, c], dof, N_CAL)[2] for c, dof in enumerate(consistency.nees_dof(18))]
    assert all(ok), ok


# ---- 3. fbus_ekf.consistency -----------------------------------------------------------------------------------------------------------
def test_anees_interval():
    for dof in (3, 6, 15, 18):
        lo, hi = consistency.anees_interval(dof, 1, 0.95)
        assert lo == pytest.approx(gating.chi2_ppf(0.025, dof), rel=1e-12) and hi == pytest.approx(gating.chi2_ppf(0.975, dof), rel=1e-12)
        for n in (1, 7, 8192):
            lo, hi = consistency.anees_interval(dof, n, 0.9)
            assert lo < dof < hi
        lo, hi = consistency.anees_interval(dof, 8192, 0.95)
        z = 1.959963984540054
        assert abs(lo - (dof - z * math.sqrt(2 * dof / 8192))) <= 1e-3 * dof
        assert abs(hi - (dof + z * math.sqrt(2 * dof / 8192))) <= 1e-3 * dof
    lo, hi = consistency.anees_interval(18, 8192)
    assert abs(lo - 17.870) < 1e-3 and abs(hi - 18.130) < 1e-3
    with pytest.raises(ValueError):
        consistency.anees_interval(0, 10)
    with pytest.raises(ValueError):
        consistency.anees_interval(3, 10, 1.0)


def test_anees_and_summary_with_nan_rows_and_a_skip_mask(cal):
    nees = cal[3][0][:1000].copy()
    assert consistency.NEES_NAMES == ("full", "pose", "p", "v", "theta", "ba", "bg", "g")
    assert consistency.nees_dof(18) == (18, 6, 3, 3, 3, 3, 3, 3) and consistency.nees_dof(15) == (15, 6, 3, 3, 3, 3, 3, 0)
    nees[3, :] = np.nan
    nees[5, capi.NEES_BG] = np.nan
    nees[7, capi.NEES_FULL] = np.inf
    skip = np.zeros(1000, np.uint8)
    skip[10:20] = 1
    nees[10:20] = 0.0
    mean, out = consistency.anees(nees, skip)
    keep = np.ones(1000, bool); keep[3] = False; keep[10:20] = False
    assert list(out) == [12, 11, 11, 11, 11, 11, 12, 11]
    k0 = keep.copy(); k0[7] = False
    assert mean[0] == pytest.approx(nees[k0, 0].mean(), rel=1e-14)
    assert mean[2] == pytest.approx(nees[keep, 2].mean(), rel=1e-14)
    s = consistency.summary(nees, 18, 0.95, skip)
    assert list(s) == list(consistency.NEES_NAMES)
    assert s["full"]["n"] == 988 and s["full"]["dof"] == 18 and s["full"]["mean"] == mean[0]
    assert (s["full"]["lo"], s["full"]["hi"]) == consistency.anees_interval(18, 988, 0.95)
    assert s["full"]["inside"] == (s["full"]["lo"] <= mean[0] <= s["full"]["hi"])
    over = consistency.summary(4.0 * nees, 18, 0.95, skip)              # an over-confident bank: P four times too small
    assert over["full"]["inside"] is False and over["p"]["inside"] is False
    s15 = consistency.summary(np.where(np.arange(8) == 7, 0.0, nees), 15)
    assert s15["g"]["inside"] is None and s15["g"]["dof"] == 0
    m, o = consistency.anees(np.full((4, 8), np.nan))
    assert np.isnan(m).all() and list(o) == [4] * 8
    with pytest.raises(ValueError):
        consistency.anees(np.zeros((4, 7)))


# ---- 4. the symbols --------------------------------------------------------------------------------------------------------------------
def test_the_two_symbols_are_declared_exported_prototyped_and_refuse_a_null_handle():
    declared = capi.declared_symbols()
    lib = capi.load_library()
    truth = (C.c_double * 19)()
    out = (C.c_double * 18)()
    for n in ("fbus_ekf_nees", "fbus_ekf_nees_dev"):
        assert n in declared, n
        assert hasattr(lib, n), n
        assert getattr(lib, n).argtypes is not None and len(getattr(lib, n).argtypes) == 6, n
        assert getattr(lib, n)(None, truth, None, out, out, out) == 1
        assert getattr(lib, n)(None, None, None, None, None, None) == 1
    assert capi.ABI_VERSION == 8 and lib.fbus_ekf_abi_version() == 8
    assert capi.NEES_COLS == 8
    assert (capi.NEES_FULL, capi.NEES_POSE, capi.NEES_P, capi.NEES_V, capi.NEES_THETA, capi.NEES_BA, capi.NEES_BG, capi.NEES_G) == tuple(range(8))
