#!/usr/bin/env python3
"""Cost of the per-marker screen (fbus_ekf_screen_markers_dev) beside the update it precedes, on one handle: B = 65 536 fp32 filters,
N = 18, first M = 4 with every slot in view, then M = 16 with 4 slots in view (the other 12 hold id -1).  Kinds: pixels left, pixels
stereo, corners (refractive triangulation of the same image points), pose.  Three launches -- the screen, the _nis_dev update of the same
frame (one wave per tile, the form that gates the survivors) and the plain _dev update (the handle's own route) -- ALTERNATED in one
process and timed with device events on the handle's stream; the state is reset from a device copy before every update (the screen
writes no record).  The bytes per filter the screen moves are counted from the code (csrc/ekf_screen.hpp: the chunks of p, q, R and those
that hold an element of P(J, J); per slot the id and the three outputs, per slot in view the measurement; kept) and printed with the
implied rate.
Prints one JSON line per (kind, M): median, min and max microseconds per launch.
  python tools/time_screen.py [--batch 65536] [--reps 40] [--warmup 5]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fbus-ekf_amd"))

# 16-byte record chunks the screen kernels load per filter: p, q, R (Rec::CH_PQR) + the covariance chunks with chunk_sel == SEL_JJ in front
# of late_start (csrc/ekf_meas.hpp), by (dtype, N)
RECORD_CHUNKS = {(32, 18): 4 + 15, (32, 15): 4 + 12, (64, 18): 8 + 16, (64, 15): 8 + 15}
MEAS_ELEMS = {"pixels_left": 8, "pixels_stereo": 16, "corners": 16, "pose": 7}


def screen_bytes_per_filter(dtype, N, kind, M, in_view):
    """loads + stores of one screen launch per filter: every slot's id, the measurement of the slots in view alone (a slot that is
    padding for the whole wave is not fetched), every slot's three outputs, kept"""
    es = 4 if dtype == 32 else 8
    return RECORD_CHUNKS[(dtype, N)] * 16 + M * 4 + in_view * MEAS_ELEMS[kind] * es + M * (4 + es + 4) + 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import torch
    from fbus_ekf import BatchedFilter, capi, synth
    assert torch.cuda.is_available(), "time_screen.py measures on a GPU"
    dev = torch.device("cuda:0")
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    B, N, dtype = args.batch, 18, 32
    prm = capi.default_params(0)
    prm.marker_size = 0.28
    nom, rot, ids4, left4, right4 = synth.pixel_wall_scene(B, 4, prm, 0.28, stereo=True)        # (replaces the map by the 16-marker wall)
    _, _, P, prev = synth.initial_state(0, B, list(prm.p0_diag), N, mixed_cov=True)
    pid4, pos4, quat4 = synth.marker_frame(0, B, 0, 4, nom, prm)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    upi = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(dev)
    stream = torch.cuda.Stream(dev)

    def spread(x, M, fill):
        """M = 4: as it is; M = 16: the four slots at 1, 6, 11, 12, the rest `fill`"""
        if M == 4:
            return x
        out = np.full((B, M) + x.shape[2:], fill, x.dtype)
        out[:, [1, 6, 11, 12]] = x
        return out
    with BatchedFilter(B, prm, device=0, dtype=dtype, nstate=N, stream=stream) as flt:
        flt.order_streams = False
        flt.set_state(nom, rot, P, prev)
        lib, h = flt._lib, flt._h
        n_d, r_d, P_d, pv_d = up(nom), up(rot), up(P), upi(prev)
        for M in (4, 16):
            o_ids = torch.empty((B, M), dtype=torch.int32, device=dev)
            o_nis = torch.empty((B, M), dtype=torch.float32, device=dev)
            o_dof = torch.empty((B, M), dtype=torch.int32, device=dev)
            o_kept = torch.empty(B, dtype=torch.int32, device=dev)
            u_nis = torch.empty(B, dtype=torch.float32, device=dev)
            u_dof = torch.empty(B, dtype=torch.int32, device=dev)
            di, dl, dr = upi(spread(ids4, M, -1)), up(spread(left4, M, 0.0)), up(spread(right4, M, 0.0))
            dpi, dpp, dpq = upi(spread(pid4, M, -1)), up(spread(pos4, M, 0.0)), up(spread(quat4, M, 0.0))
            torch.cuda.synchronize()
            G, S = capi.VIS_REFRACTIVE, capi.MODE_STACKED
            outs = (p(o_ids), p(o_nis), p(o_dof), p(o_kept))
            cases = {
                "pixels_left": (lambda: lib.fbus_ekf_screen_markers_dev(h, capi.SCREEN_PIXELS, M, p(di), p(dl), None, G, None, *outs),
                                lambda: lib.fbus_ekf_correct_pixels_nis_dev(h, M, p(di), p(dl), None, None, p(u_nis), p(u_dof)),
                                lambda: lib.fbus_ekf_correct_pixels_dev(h, M, p(di), p(dl), None, None)),
                "pixels_stereo": (lambda: lib.fbus_ekf_screen_markers_dev(h, capi.SCREEN_PIXELS, M, p(di), p(dl), p(dr), G, None, *outs),
                                  lambda: lib.fbus_ekf_correct_pixels_nis_dev(h, M, p(di), p(dl), p(dr), None, p(u_nis), p(u_dof)),
                                  lambda: lib.fbus_ekf_correct_pixels_dev(h, M, p(di), p(dl), p(dr), None)),
                "corners": (lambda: lib.fbus_ekf_screen_markers_dev(h, capi.SCREEN_CORNERS, M, p(di), p(dl), p(dr), G, None, *outs),
                            lambda: lib.fbus_ekf_correct_corners_nis_dev(h, M, p(di), p(dl), p(dr), G, S, None, p(u_nis), p(u_dof)),
                            lambda: lib.fbus_ekf_correct_corners_dev(h, M, p(di), p(dl), p(dr), G, S, None)),
                "pose": (lambda: lib.fbus_ekf_screen_markers_dev(h, capi.SCREEN_POSE, M, p(dpi), p(dpp), p(dpq), G, None, *outs),
                         lambda: lib.fbus_ekf_correct_nis_dev(h, M, p(dpi), p(dpp), p(dpq), S, None, p(u_nis), p(u_dof)),
                         lambda: lib.fbus_ekf_correct_dev(h, M, p(dpi), p(dpp), p(dpq), S, None)),
            }
            for kind, launches in cases.items():
                times = {k: [] for k in ("screen", "update_nis", "update")}
                for rep in range(args.warmup + args.reps):
                    for k, fn in zip(times, launches):
                        if k != "screen":
                            assert lib.fbus_ekf_set_state_dev(h, p(n_d), p(r_d), p(P_d), p(pv_d)) == 0
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(stream)
                        assert fn() == 0
                        e1.record(stream)
                        e1.synchronize()
                        if rep >= args.warmup:
                            times[k].append(e0.elapsed_time(e1) * 1e3)
                judged = float((o_dof > 0).float().sum(dim=1).mean())
                per = screen_bytes_per_filter(dtype, N, kind, M, 4)
                med = {k: float(np.median(v)) for k, v in times.items()}
                print(json.dumps({"kind": kind, "M": M, "B": B, "judged_slots_per_filter": round(judged, 2),
                                  "screen_bytes_per_filter": per, "screen_TB_per_s": round(per * B / med["screen"] / 1e6, 3),
                                  "screen_over_update_nis": round(med["screen"] / med["update_nis"], 3),
                                  "us": {k: {"median": round(med[k], 2), "min": round(min(v), 2), "max": round(max(v), 2)}
                                         for k, v in times.items()}}), flush=True)


if __name__ == "__main__":
    main()
