"""CPU suite of the predicted corner pixels (include/fbus_ekf.h, fbus_ekf_project_markers*; added under FBUS_ABI_VERSION 8 without a
bump): the two symbols, their prototypes and null-handle checks, the unit that builds the kernels, the Python and C++ layers, the search
window, and the reference's closed-form in-view rule against the oracle's own verdict on the scene of the GPU suite."""
import ctypes as C
import importlib.util
import math
import os
import re

import numpy as np
import pytest

import oracle_capi as oc
import project_ref
import support
from fbus_ekf import capi, gating

NEW = ["fbus_ekf_project_markers", "fbus_ekf_project_markers_dev"]


def test_the_two_symbols_are_declared_exported_prototyped_and_refuse_a_null_handle():
    declared = capi.declared_symbols()
    lib = capi.load_library()
    for n in NEW:
        assert n in declared, n
        assert hasattr(lib, n), n
        assert getattr(lib, n).argtypes is not None and len(getattr(lib, n).argtypes) == 10, n
    assert capi.ABI_VERSION == 8 and lib.fbus_ekf_abi_version() == 8
    ids = (C.c_int32 * 4)()
    buf = (C.c_double * 64)()
    for n in NEW:
        for cameras in (1, 2, 3):
            assert getattr(lib, n)(None, 1, ids, cameras, None, buf, buf, buf, buf, None) == 1
        assert getattr(lib, n)(None, 0, None, 2, None, None, None, None, None, None) == 1


def test_the_kernel_builds_in_the_screen_family_unit(repo_root):
    spec = importlib.util.spec_from_file_location("fbus_build_project", os.path.join(repo_root, "fbus-ekf_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert any(h.endswith("ekf_project.hpp") for h in b.HEADERS)            # a change of the kernel rebuilds the library
    csrc = os.path.join(repo_root, "fbus-ekf_amd", "csrc")
    code = b.FAMILIES["screen"][0]
    tu = open(os.path.join(csrc, "small_tu.hip")).read()
    # the family's block: the new header directly in front of ekf_screen.hpp, and in no other family's
    assert f'#elif FBUS_TU_FAMILY == {code}\n#include "ekf_project.hpp"\n#include "ekf_screen.hpp"\n' in tu
    assert tu.count('#include "ekf_project.hpp"') == 1
    for cam in (1, 2):
        assert f"FBUS_INST(launch_project_k<FBUS_TN, {cam}>)" in tu
    assert "launch_project_k" in open(os.path.join(csrc, "ekf_launch.hpp")).read()
    main = open(os.path.join(csrc, "fbus_ekf.hip")).read()
    assert '#include "ekf_project.hpp"' not in main                         # the host unit holds no kernel
    assert len(b.units()) == 82                                             # no unit of its own


def test_the_python_and_cxx_layers_carry_the_method(repo_root):
    from fbus_ekf import BatchedFilter, consistency
    assert callable(BatchedFilter.project_markers)
    assert callable(consistency.observe) and callable(gating.search_window)
    hdr = open(os.path.join(repo_root, "include", "fbus", "batched_filter.hpp")).read()
    for m in ("project_markers", "project_markers_dev"):
        assert f"void {m}(" in hdr, m
    text = open(os.path.join(repo_root, "include", "fbus_ekf.h")).read()
    assert "H P_JJ H' + r_pix I_2" in text and "klim = 0.81 a1^2 / (1 - a1^2)" in text


@pytest.mark.parametrize("prob", [0.5, 0.95, 0.997])
def test_search_window_is_the_box_around_the_chi_square_ellipse(prob):
    k = gating.chi2_ppf(prob, 2)
    assert abs(k - (-2.0 * math.log(1.0 - prob))) <= 1e-10 * k            # two degrees of freedom: the closed form
    cov = np.array([[[4e-6, 1e-6, 9e-6], [0.0, 0.0, 0.0]], [[1e-4, -3e-5, 2.5e-5], [1.0, 0.0, 1.0]]])
    w = gating.search_window(cov, prob)
    assert w.shape == (2, 2, 2)
    assert np.allclose(w, np.sqrt(k * cov[..., [0, 2]]), rtol=1e-15, atol=0)
    assert np.all(w[0, 1] == 0.0)                                           # not in view: no window
    assert np.allclose(w[1, 1], math.sqrt(-2.0 * math.log(1.0 - prob)), rtol=1e-10)
    # the box holds the ellipse: its extreme point along u is sqrt(k S_uu)
    S = np.array([[1e-4, -3e-5], [-3e-5, 2.5e-5]])
    th = np.linspace(0, 2 * np.pi, 2001)
    pts = np.linalg.cholesky(S) @ (math.sqrt(k) * np.stack([np.cos(th), np.sin(th)]))
    assert np.all(np.abs(pts[0]) <= w[1, 0, 0] * (1 + 1e-12)) and np.all(np.abs(pts[1]) <= w[1, 0, 1] * (1 + 1e-12))
    assert np.abs(pts[0]).max() >= w[1, 0, 0] * (1 - 1e-5)


@pytest.mark.parametrize("tilted", [False, True])
def test_the_reference_in_view_flags_equal_the_oracle_verdict_on_the_scene(tilted):
    """every marker of the map, listed or not, seen from every filter of the GPU suite's scene: the closed form of the header's rule 2
    against the ok of the oracle's projection, per camera (left alone, and left and right together)"""
    prm, nom, rot, _, _, ids, _, _ = support.perturbed_setup(130, 64, 18, 0, "stereo", M=4, seed=3, n=64, tilted=tilted)
    vp = support.vp_tilted() if tilted else oc.vision_params()
    nmap = prm.n_markers
    X = np.array([[project_ref.corners_cam(nom[b, 0:3], rot[b].reshape(3, 3), prm, k) for k in range(nmap)] for b in range(130)])
    f = project_ref.in_view(X, prm)                                          # (130, nmap, 4, 2)
    flat = X.reshape(-1, 3)
    okL = oc.project_stereo(vp, flat, stereo=False)[2].reshape(f.shape[:-1])
    okLR = oc.project_stereo(vp, flat, stereo=True)[2].reshape(f.shape[:-1])
    assert np.array_equal(f[..., 0], okL)
    assert np.array_equal(f[..., 0] & f[..., 1], okLR)
    assert f.any() and not f.all()
    # what the GPU suite relies on: every listed corner is in view of both cameras
    listed = np.array([[project_ref.slot_of(prm, int(m)) for m in row] for row in ids])
    for b in range(130):
        for k in listed[b][listed[b] >= 0]:
            assert f[b, k].all(), (b, k)
