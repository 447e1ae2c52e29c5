"""CPU suite for per-filter process and measurement noise (fbus_ekf_set_noise, include/fbus_ekf.h): the three symbols and their
null-handle checks, the unchanged ABI version, and the table helpers of fbus_ekf.noise (shapes, round-robin assignment, column
order against the fbus_params fields)."""
import ctypes as C

import numpy as np
import pytest

from fbus_ekf import capi, noise

NEW = ["fbus_ekf_set_noise", "fbus_ekf_set_noise_dev", "fbus_ekf_get_noise"]


def test_new_symbols_are_declared_exported_and_refuse_a_null_handle():
    declared = capi.declared_symbols()
    lib = capi.load_library()
    for n in NEW:
        assert n in declared, n
        assert hasattr(lib, n), n
    tab = (C.c_double * capi.NOISE_COLS)(*([1e-3] * capi.NOISE_COLS))
    assert lib.fbus_ekf_set_noise(None, tab) == 1
    assert lib.fbus_ekf_set_noise(None, None) == 1
    assert lib.fbus_ekf_set_noise_dev(None, None) == 1
    assert lib.fbus_ekf_get_noise(None, tab) == 1


def test_abi_version_is_unchanged():
    lib = capi.load_library()
    assert capi.ABI_VERSION == 8 and lib.fbus_ekf_abi_version() == 8
    assert capi.NOISE_COLS == 7 == len(noise.COLUMNS)
    hdr = open(capi._HEADER).read()
    assert "#define FBUS_NOISE_COLS 7" in hdr


def test_columns_are_the_params_fields_in_order():
    prm = capi.default_params(capi.DIALECT_CPP)
    prm.q_diag[0], prm.q_diag[1], prm.q_diag[2], prm.q_diag[3] = 1.0, 2.0, 3.0, 4.0
    prm.r_pos, prm.r_quat, prm.r_pix = 5.0, 6.0, 7.0
    assert noise.COLUMNS == ("q_v", "q_theta", "q_ba", "q_bg", "r_pos", "r_quat", "r_pix")
    np.testing.assert_array_equal(noise.row_of(prm), np.arange(1.0, 8.0))
    # the header names the same columns in the same order
    hdr = open(capi._HEADER).read()
    assert "q_v q_theta q_ba q_bg r_pos r_quat r_pix" in hdr
    # and the params struct holds those fields
    names = [f for f, _ in capi.FbusParams._fields_]
    for f in ("q_diag", "r_pos", "r_quat", "r_pix"):
        assert f in names


def test_from_params_broadcasts_one_row():
    prm = capi.default_params()
    t = noise.from_params(prm, 37)
    assert t.shape == (37, 7) and t.dtype == np.float64
    np.testing.assert_array_equal(t, np.tile(noise.row_of(prm), (37, 1)))


@pytest.mark.parametrize("B", [1, 5, 4197])
def test_grid_is_the_cartesian_product_assigned_round_robin(B):
    prm = capi.default_params()
    base = noise.row_of(prm)
    table, hyp, rows = noise.grid(prm, B, r_pix=[0.5, 1.0, 2.0], q_v=[0.1, 10.0])
    assert table.shape == (B, 7) and hyp.shape == (B,) and rows.shape == (6, 7)
    np.testing.assert_array_equal(hyp, np.arange(B) % 6)
    np.testing.assert_array_equal(table, rows[hyp])
    # product order: q_v (first in COLUMNS) outer, r_pix inner; other columns keep the params' values
    iq, ip = noise.COLUMNS.index("q_v"), noise.COLUMNS.index("r_pix")
    k = 0
    for fq in (0.1, 10.0):
        for fp in (0.5, 1.0, 2.0):
            assert rows[k, iq] == base[iq] * fq and rows[k, ip] == base[ip] * fp
            others = [c for c in range(7) if c not in (iq, ip)]
            np.testing.assert_array_equal(rows[k, others], base[others])
            k += 1
    # no factors: one hypothesis, the params' own row
    t1, h1, r1 = noise.grid(prm, B)
    assert r1.shape == (1, 7) and not h1.any()
    np.testing.assert_array_equal(t1, noise.from_params(prm, B))


def test_grid_refuses_unknown_columns():
    with pytest.raises(ValueError):
        noise.grid(capi.default_params(), 4, r_foo=[1.0])
