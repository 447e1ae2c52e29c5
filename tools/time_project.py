#!/usr/bin/env python3
"""Cost of the predicted corner pixels (fbus_ekf_project_markers_dev) beside the kernels that form the same projections, on one handle:
B = 65 536 filters, N = 18, fp32 and fp64 records, left camera and stereo, first M = 4 with every slot in view, then M = 16 with 4 slots in
view (the other 12 hold id -1).  Four launches ALTERNATED in one process and timed with device events on the handle's stream: the
projection with its image points alone (`project_uv`: left / right, no covariance, no view), the projection with every output
(`project_all`), the unchanged screen_markers_dev(PIXELS) of the same frame (the same projections plus two 6 x 6 factorisations per
slot) and correct_pixels_dev (the handle's own route; the state is reset from a device copy before it -- the other three write no
record).  The bytes per filter the projection moves are counted from the code (csrc/ekf_project.hpp: the chunks of p, q, R, with a
covariance those that hold an element of P(J, J); per slot the id and the outputs) and printed with the implied rate.
One child process per (dtype, cameras) case, each under its own time limit; one JSON line per (case, M): median, min and max microseconds.
  python tools/time_project.py [--batch 65536] [--reps 40] [--warmup 5] [--limit 120]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fbus-ekf_amd"))

# 16-byte record chunks per filter: p, q, R (Rec::CH_PQR), and the covariance chunks with chunk_sel == SEL_JJ (csrc/ekf_meas.hpp), by dtype (N = 18)
PQR_CHUNKS = {32: 4, 64: 8}
JJ_CHUNKS = {32: 15, 64: 16}


def project_bytes_per_filter(dtype, M, cameras, full):
    """loads + stores of one launch per filter"""
    es = 4 if dtype == 32 else 8
    rd = (PQR_CHUNKS[dtype] + (JJ_CHUNKS[dtype] if full else 0)) * 16 + M * 4
    wr = M * cameras * 8 * es + (M * cameras * 96 + M if full else 0)
    return rd, wr


def one_case(args, dtype, cameras):
    import torch
    from fbus_ekf import BatchedFilter, capi, synth
    assert torch.cuda.is_available(), "time_project.py measures on a GPU"
    dev = torch.device("cuda:0")
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    B, N = args.batch, 18
    npd, tt = (np.float32, torch.float32) if dtype == 32 else (np.float64, torch.float64)
    prm = capi.default_params(0)
    prm.marker_size = 0.28
    nom, rot, ids4, left4, right4 = synth.pixel_wall_scene(B, 4, prm, 0.28, stereo=True)        # (replaces the map by the 16-marker wall)
    _, _, P, prev = synth.initial_state(0, B, list(prm.p0_diag), N, mixed_cov=True)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, npd)).to(dev)
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
            o_l, o_r = torch.empty((B, M, 8), dtype=tt, device=dev), torch.empty((B, M, 8), dtype=tt, device=dev)
            o_cl, o_cr = (torch.empty((B, M, 4, 3), dtype=torch.float64, device=dev) for _ in range(2))
            o_v = torch.empty((B, M), dtype=torch.uint8, device=dev)
            s_ids, s_dof = (torch.empty((B, M), dtype=torch.int32, device=dev) for _ in range(2))
            s_nis = torch.empty((B, M), dtype=tt, device=dev)
            s_kept = torch.empty(B, dtype=torch.int32, device=dev)
            di, dl = upi(spread(ids4, M, -1)), up(spread(left4, M, 0.0))
            dr = up(spread(right4, M, 0.0)) if cameras == 2 else None
            torch.cuda.synchronize()
            launches = {
                "project_uv": lambda: lib.fbus_ekf_project_markers_dev(h, M, p(di), cameras, None, p(o_l), p(o_r), None, None, None),
                "project_all": lambda: lib.fbus_ekf_project_markers_dev(h, M, p(di), cameras, None, p(o_l), p(o_r), p(o_cl), p(o_cr), p(o_v)),
                "screen": lambda: lib.fbus_ekf_screen_markers_dev(h, capi.SCREEN_PIXELS, M, p(di), p(dl), p(dr), capi.VIS_REFRACTIVE, None,
                                                                  p(s_ids), p(s_nis), p(s_dof), p(s_kept)),
                "update": lambda: lib.fbus_ekf_correct_pixels_dev(h, M, p(di), p(dl), p(dr), None),
            }
            times = {k: [] for k in launches}
            for rep in range(args.warmup + args.reps):
                for k, fn in launches.items():
                    if k == "update":
                        assert lib.fbus_ekf_set_state_dev(h, p(n_d), p(r_d), p(P_d), p(pv_d)) == 0
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    assert fn() == 0
                    e1.record(stream)
                    e1.synchronize()
                    if rep >= args.warmup:
                        times[k].append(e0.elapsed_time(e1) * 1e3)
            in_view = float(sum(((o_v >> k) & 1).float().sum() for k in range(8))) / B
            med = {k: float(np.median(v)) for k, v in times.items()}
            rd_uv, wr_uv = project_bytes_per_filter(dtype, M, cameras, False)
            rd_all, wr_all = project_bytes_per_filter(dtype, M, cameras, True)
            print(json.dumps({"dtype": dtype, "cameras": cameras, "M": M, "B": B, "projections_in_view_per_filter": round(in_view, 2),
                              "bytes_per_filter": {"uv": [rd_uv, wr_uv], "all": [rd_all, wr_all]},
                              "TB_per_s": {"uv": round((rd_uv + wr_uv) * B / med["project_uv"] / 1e6, 3),
                                           "all": round((rd_all + wr_all) * B / med["project_all"] / 1e6, 3)},
                              "project_uv_over_screen": round(med["project_uv"] / med["screen"], 3),
                              "us": {k: {"median": round(med[k], 2), "min": round(min(v), 2), "max": round(max(v), 2)}
                                     for k, v in times.items()}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--limit", type=int, default=120, help="seconds per case")
    ap.add_argument("--case", default=None, help="(internal) dtype,cameras: run this case in this process")
    args = ap.parse_args()
    if args.case:
        dtype, cameras = (int(x) for x in args.case.split(","))
        return one_case(args, dtype, cameras)
    for dtype in (32, 64):
        for cameras in (1, 2):
            cmd = [sys.executable, os.path.abspath(__file__), "--batch", str(args.batch), "--reps", str(args.reps), "--warmup", str(args.warmup),
                   "--case", f"{dtype},{cameras}"]
            try:
                rc = subprocess.run(cmd, timeout=args.limit).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc != 0:                         # (nothing more is started on the device behind a case that failed)
                print(json.dumps({"dtype": dtype, "cameras": cameras, "failed": rc}), flush=True)
                return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
