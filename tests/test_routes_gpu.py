"""GPU suite: the route of every frame and window entry point (fbus-ekf_amd/csrc/ekf_route.hpp), pinned by what can be
observed from outside -- B = 128 filters, the handle placed in each size class with set_policy_batch.

For every cell (handle state x size class x entry point x call shape):
  1 signature   the launch counts of timing_read are the ones the route implies: a per-call frame counts its predict_n (predict for
                K = 1) and its update, every fused or resident route counts the frame kind only, a window counts its F frames
  2 frames      the records and applied flags after a window == after the same frames one by one through the single-frame entry point,
                bit for bit (team windows against team frames, one-wave against one-wave, per-call against per-call)
The expected route is restated in tests/route_cells.py from the documented rules and the handle's own launch_info answers; the last test
checks that the cells reach every value of both route enums."""
import numpy as np
import pytest

from fbus_ekf import capi
from route_cells import CFGS, KINDS, NEAREST, STACKED, data_of, frame_route, make, one_frame, shapes_of, window, window_route
from support import same_state

pytestmark = pytest.mark.gpu


def signature(route, kind, M, K):
    """{kernel kind: launches counted} of one frame"""
    n = dict.fromkeys(KINDS, 0)
    if route == "per_call":
        if K > 0:
            n[capi.KERNEL_PREDICT if K == 1 else capi.KERNEL_PREDICT_N] = 1
        if M > 0:
            n[capi.KERNEL_CORRECT if kind == "pose" else capi.KERNEL_CORRECT_CORNERS] = 1
    else:
        n[capi.KERNEL_FRAME] = 1
    return n


def counts(f):
    return {k: f.timing_read(k)[1] for k in KINDS}


def total(parts):
    return {k: sum(p[k] for p in parts) for k in KINDS}


@pytest.mark.parametrize("cfg", CFGS, ids=repr)
def test_window_signature_and_window_equals_its_frames(cfg):
    d = data_of(cfg)
    for kind, mode, M, kc, rows in shapes_of(cfg):
        what = f"{cfg}: {kind} mode {mode} M {M} kcount {kc} rows {rows}"
        with make(cfg, d, kind != "pose") as w, make(cfg, d, kind != "pose") as s:
            routes = [frame_route(w, cfg, kind, mode, M, K) for K in kc]
            expect = total([signature(r, kind, M, K) for r, K in zip(routes, kc)])
            window(w, d, kind, mode, M, kc, rows)
            w.sync()
            assert counts(w) == expect, what
            k0 = 0
            for fr, K in enumerate(kc):
                one_frame(s, d, kind, mode, M, K, fr, k0)
                k0 += K
            s.sync()
            assert counts(s) == expect, what
            assert same_state(w.get_state(), s.get_state()) and np.array_equal(w.applied(), s.applied()), what


@pytest.mark.parametrize("cfg", [CFGS[i] for i in (0, 1, 7, 8, 12)], ids=repr)
def test_single_frame_signature_at_the_sample_count_boundaries(cfg):
    """K = 255 is the last count of the resident and team kernels (a byte); K = 0 has no predict, M = 0 no update"""
    d = data_of(cfg)
    for kind, mode, M in (("pose", STACKED, 4), ("pose", STACKED, 0), ("stereo", STACKED, 4), ("corners", NEAREST, 1), ("left", STACKED, 0)):
        for K in (0, 1, 255, 256):
            with make(cfg, d, kind != "pose") as f:
                r = frame_route(f, cfg, kind, mode, M, K)
                one_frame(f, d, kind, mode, M, K)
                f.sync()
                assert counts(f) == signature(r, kind, M, K), f"{cfg}: {kind} mode {mode} M {M} K {K}: {r}"


def test_the_cells_reach_every_route():
    """the walks above visit every value of both route enums (asked of the handles, nothing launched)"""
    frames, windows = set(), set()
    for cfg in CFGS:
        with make(cfg, data_of(cfg), False) as f:
            for kind, mode, M, kc, rows in shapes_of(cfg):
                windows.add(window_route(f, cfg, kind, mode, M, len(kc), rows))
                frames.update(frame_route(f, cfg, kind, mode, M, K) for K in kc)
    assert frames == {"per_call", "f64_fused", "fused", "team", "tabled_resident", "meas_resident"}
    assert windows == {"one_wave", "team", "team_frames", "by_frame"}
