#!/usr/bin/env python3
"""Cost of a per-filter noise table (fbus_ekf_set_noise) at B = 65 536 filters, fp32 records, N = 18: each route without a table (the
twin) and with one (5 rows round-robin, x0.1 .. x10 of the defaults), ALTERNATED in one process on one handle (the table switched on and
off through the device form) and timed with HIP events on the handle's stream; the state is reset from a device copy before every launch.
Cases: predict, predict_n K = 7, pose stacked M = 4, pixels left M = 4 and 16, pixels stereo M = 4, corners (3-D) stacked M = 4, and two
30-frame windows, K = 7 per frame (host wall time around the call): frames_meas (pixels left M = 4) and frames (pose rows, stacked, M = 4).
The windows take a third variant, alternated with the other two: the table with fbus_ekf_set_policy_batch(h, 64) -- below half a chip a
tabled window runs frame by frame through the tabled one-wave per-call kernels, the route every tabled window took before the resident
kernels read the table; above it (the handle's own 65 536 filters) the table variant is the resident window.
Prints one JSON line per case: median and min / max per variant, the table's overhead against the twin; for the windows also whether the
resident table variant's max lies below the frame-by-frame variant's min.
  python tools/time_noise.py [--batch 65536] [--reps 30] [--warmup 3] [--only frames_]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fbus-ekf_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="", help="run the cases whose name contains this string")
    args = ap.parse_args()
    import torch
    from fbus_ekf import BatchedFilter, capi, noise, synth
    dev = torch.device("cuda:0")
    B = args.batch
    prm = capi.default_params(0)
    nom, rot, P, prev = synth.initial_state(0, B, list(prm.p0_diag), 18, mixed_cov=True)
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    table, _, _ = noise.grid(prm, B, q_v=[0.1, 10.0], r_pix=[0.3, 3.0], r_pos=[1.0, 0.5])
    tab_d = torch.from_numpy(table).to(dev)
    K, F = 7, 30
    acc, gyr = synth.imu_samples(0, B, 0, K * F, nom)
    da, dg = f32(acc), f32(gyr)
    ddt = f32(np.full(K * F, 0.005))
    rng = np.random.default_rng(1)
    cases = [("predict", "predict", 0, False), ("predict_n_k7", "predict_n", 0, False), ("pose_stacked_m4", "pose", 4, False),
             ("pixels_left_m4", "pixels", 4, False), ("pixels_left_m16", "pixels", 16, False), ("pixels_stereo_m4", "pixels", 4, True),
             ("corners_stacked_m4", "corners", 4, False), ("frames_meas_30x_left_m4", "window", 4, False),
             ("frames_30x_stacked_m4", "posewindow", 4, False)]
    cases = [c for c in cases if args.only in c[0]]
    kernel_of = {"predict": capi.KERNEL_PREDICT, "predict_n": capi.KERNEL_PREDICT_N, "pose": capi.KERNEL_CORRECT,
                 "pixels": capi.KERNEL_CORRECT_CORNERS, "corners": capi.KERNEL_CORRECT_CORNERS}
    with BatchedFilter(B, prm, device=0, dtype=32, nstate=18) as flt:
        flt.order_streams = False
        flt.set_state(nom, rot, P, prev)
        lib, h = flt._lib, flt._h
        n_d, r_d, P_d, pv_d = f32(nom), f32(rot), f32(P), torch.from_numpy(np.ascontiguousarray(prev, np.int32)).to(dev)
        for name, kind, M, stereo in cases:
            if M:
                ids = np.broadcast_to(np.resize(synth.marker_table(prm)[0], M), (B, M))     # every slot a map marker
                if kind in ("pose", "posewindow"):
                    ids, pos, quat = synth.marker_frame(0, B, 0, M, nom, prm)
                    dp, dq = f32(pos), f32(quat)
                left = f32(rng.uniform(-0.3, 0.3, (B, M, 12 if kind == "corners" else 8)))
                right = f32(rng.uniform(-0.3, 0.3, (B, M, 8))) if stereo else None
                di = torch.from_numpy(np.ascontiguousarray(ids, np.int32)).to(dev)
                if kind in ("window", "posewindow"):
                    wi = di.repeat(F, 1)
                    wl = left.repeat(F, 1, 1)
                    kc = (C.c_int32 * F)(*([K] * F))
                if kind == "posewindow":
                    wp, wq = dp.repeat(F, 1, 1), dq.repeat(F, 1, 1)

            def call():
                if kind == "predict":
                    return lib.fbus_ekf_predict_dev(h, p(da), p(dg), p(ddt), 0)
                if kind == "predict_n":
                    return lib.fbus_ekf_predict_n_dev(h, K, p(da), p(dg), p(ddt), 0)
                if kind == "pose":
                    return lib.fbus_ekf_correct_dev(h, M, p(di), p(dp), p(dq), capi.MODE_STACKED, None)
                if kind == "pixels":
                    return lib.fbus_ekf_correct_pixels_dev(h, M, p(di), p(left), p(right), None)
                if kind == "corners":
                    return lib.fbus_ekf_correct_corners_dev(h, M, p(di), p(left), None, capi.VIS_CORNERS3D, capi.MODE_STACKED, None)
                if kind == "posewindow":
                    return lib.fbus_ekf_frames_fused_dev(h, F, kc, p(da), p(dg), p(ddt), 0, M, p(wi), p(wp), p(wq), capi.MODE_STACKED, None)
                return lib.fbus_ekf_frames_meas_fused_dev(h, F, kc, p(da), p(dg), p(ddt), 0, capi.MEAS_PIXELS, M, p(wi), p(wl), None,
                                                          capi.VIS_REFRACTIVE, capi.MODE_STACKED, None)
            window = kind in ("window", "posewindow")
            times = {"twin": [], "table": [], "table_frame_by_frame": []} if window else {"twin": [], "table": []}
            for rep in range(args.warmup + args.reps):
                for k in times:
                    assert lib.fbus_ekf_set_noise_dev(h, p(tab_d) if k != "twin" else None) == 0
                    flt.set_policy_batch(64 if k == "table_frame_by_frame" else 0)
                    if window:
                        assert flt.launch_info(capi.INFO_NOISE_RESIDENT) == (1 if k == "table" else 0)
                    assert lib.fbus_ekf_set_state_dev(h, p(n_d), p(r_d), p(P_d), p(pv_d)) == 0
                    flt.sync()
                    if window:
                        t0 = time.perf_counter()
                        assert call() == 0
                        flt.sync()
                        us = (time.perf_counter() - t0) * 1e6
                    else:
                        flt.timing_enable(True)
                        flt.timing_reset()
                        assert call() == 0
                        flt.sync()
                        us = flt.timing_read(kernel_of[kind])[0] * 1e3
                        flt.timing_enable(False)
                    if rep >= args.warmup:
                        times[k].append(us)
            flt.set_policy_batch(0)
            med = {k: float(np.median(v)) for k, v in times.items()}
            out = {"case": name, "B": B, "us": {k: {"median": round(med[k], 2), "min": round(min(v), 2), "max": round(max(v), 2)}
                                                for k, v in times.items()},
                   "overhead_pct": round(100 * (med["table"] / med["twin"] - 1), 2)}
            if window:
                out["resident_max_below_frame_by_frame_min"] = bool(max(times["table"]) < min(times["table_frame_by_frame"]))
                out["frame_by_frame_over_resident"] = round(med["table_frame_by_frame"] / med["table"], 3)
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
