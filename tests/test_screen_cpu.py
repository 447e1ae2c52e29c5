"""CPU suite of the per-marker screen (include/fbus_ekf.h, fbus_ekf_screen_markers*; added under FBUS_ABI_VERSION 8 without a bump): the two
symbols, their prototypes and null-handle checks, the unit that builds the kernels, the Python and C++ layers, and the algebra the kernels
evaluate the per-marker statistic by -- the Cholesky factor of P_JJ once per filter, then per marker |D^-1 C' b|^2 -- restated in numpy
against r' (H P H' + R)^-1 r of one marker's rows."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest

from fbus_ekf import capi

NEW = ["fbus_ekf_screen_markers", "fbus_ekf_screen_markers_dev"]


def test_the_two_symbols_are_declared_exported_prototyped_and_refuse_a_null_handle():
    declared = capi.declared_symbols()
    lib = capi.load_library()
    for n in NEW:
        assert n in declared, n
        assert hasattr(lib, n), n
        assert getattr(lib, n).argtypes is not None and len(getattr(lib, n).argtypes) == 12, n
    assert capi.ABI_VERSION == 8 and lib.fbus_ekf_abi_version() == 8
    assert (capi.SCREEN_POSE, capi.SCREEN_PIXELS, capi.SCREEN_CORNERS) == (0, 1, 2)
    ids = (C.c_int32 * 4)()
    buf = (C.c_float * 64)()
    for n in NEW:
        for kind in (capi.SCREEN_POSE, capi.SCREEN_PIXELS, capi.SCREEN_CORNERS, 7):
            assert getattr(lib, n)(None, kind, 4, ids, buf, buf, capi.VIS_REFRACTIVE, None, ids, None, None, None) == 1
        assert getattr(lib, n)(None, capi.SCREEN_PIXELS, 0, None, None, None, 0, None, None, None, None, None) == 1


def test_the_kernel_builds_in_its_family_unit(repo_root):
    spec = importlib.util.spec_from_file_location("fbus_build_screen", os.path.join(repo_root, "fbus-ekf_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert any(h.endswith("ekf_screen.hpp") for h in b.HEADERS)            # a change of the kernel rebuilds the library
    csrc = os.path.join(repo_root, "fbus-ekf_amd", "csrc")
    units = [u for u in b.units() if u[0].endswith("_screen")]
    assert sorted(u[0] for u in units) == ["f32_15_screen", "f32_18_screen", "f64_15_screen", "f64_18_screen"]
    assert {u[1] for u in units} == {os.path.join(csrc, "small_tu.hip")}
    # the family's branch of the unit source includes the header: that unit instantiates the kernel
    code = b.FAMILIES["screen"][0]
    tu = open(os.path.join(csrc, "small_tu.hip")).read()
    assert re.search(rf'#elif FBUS_TU_FAMILY == {code}\n(?:#include "ekf_\w+\.hpp"\n)*?#include "ekf_screen.hpp"\n', tu)
    assert all(f"-DFBUS_TU_FAMILY={code}" in u[2] for u in units)
    main = open(os.path.join(csrc, "fbus_ekf.hip")).read()
    assert '#include "ekf_screen.hpp"' not in main                                  # ... and the host unit does not


def test_the_python_and_cxx_layers_carry_the_method(repo_root):
    from fbus_ekf import BatchedFilter
    assert callable(BatchedFilter.screen_markers)
    hdr = open(os.path.join(repo_root, "include", "fbus", "batched_filter.hpp")).read()
    for m in ("screen_markers", "screen_markers_dev"):
        assert f"void {m}(" in hdr, m
    assert "vision.cpp:825-853" in open(os.path.join(repo_root, "include", "fbus_ekf.h")).read()


def _rand_spd(rng, n, scale):
    A = rng.normal(size=(n, n))
    return scale * (A @ A.T + 0.1 * np.eye(n))


def _chol_drop(A):
    """lower Cholesky factor; a pivot that is not positive drops its column (the kernels' rule)"""
    n = len(A)
    Cf = np.zeros((n, n))
    for a in range(n):
        piv = A[a, a] - Cf[a, :a] @ Cf[a, :a]
        if piv > 0:
            Cf[a, a] = np.sqrt(piv)
            Cf[a + 1:, a] = (A[a + 1:, a] - Cf[a + 1:, :a] @ Cf[a, :a]) / Cf[a, a]
    return Cf


@pytest.mark.parametrize("case", ["pixels", "corners", "pose", "collinear"])
def test_the_hoisted_factor_form_equals_r_S_inverse_r_per_marker(case):
    """C = chol(P_JJ) once per filter; per marker m of the frame, from ITS rows alone:
    w sum res^2 - b' P_JJ (I + Lam P_JJ)^-1 b, evaluated as |D^-1 C' b|^2 with D D' = I + C' Lam C, against r' (H P H' + R)^-1 r of the
    marker's rows -- also for a rank-deficient Lam (a marker whose corners are collinear)"""
    rng = np.random.default_rng({"pixels": 1, "corners": 2, "pose": 3, "collinear": 4}[case])
    N, J = 18, [0, 1, 2, 6, 7, 8]
    nrow = {"pixels": 8, "corners": 12, "pose": 7, "collinear": 12}[case]
    for _ in range(10):
        P = _rand_spd(rng, N, 1e-7 if case != "pose" else 1e-4)
        PJJ = P[np.ix_(J, J)]
        Cf = _chol_drop(PJJ)
        assert np.allclose(Cf @ Cf.T, PJJ, rtol=1e-13, atol=0)
        for m in range(4):                                   # four markers of one frame share the factor
            Hj = rng.normal(size=(nrow, 6))
            if case == "collinear":
                Hj[6:] = Hj[:6] * rng.normal(size=(6, 1))
                Hj[:, 5] = 0.0
            H = np.zeros((nrow, N))
            H[:, J] = Hj
            rdiag = np.full(nrow, 1e-6) if case != "pose" else np.array([1e-4] * 3 + [1e-2] * 4)
            r = rng.normal(size=nrow) * np.sqrt(rdiag) * 3
            ref = r @ np.linalg.solve(H @ P @ H.T + np.diag(rdiag), r)
            Lam = Hj.T @ (Hj / rdiag[:, None])
            b = Hj.T @ (r / rdiag)
            sumw = np.sum(r * r / rdiag)
            direct = sumw - b @ PJJ @ np.linalg.solve(np.eye(6) + Lam @ PJJ, b)
            D = np.linalg.cholesky(np.eye(6) + Cf.T @ Lam @ Cf)
            v = np.linalg.solve(D, Cf.T @ b)
            hoisted = sumw - v @ v
            bound = 1e-12 * max(ref, 1.0) * max(1.0, sumw / ref)
            assert abs(direct - ref) <= bound, (direct, ref)
            assert abs(hoisted - ref) <= bound, (hoisted, ref)
