#!/usr/bin/env python3
"""Cost of the per-frame trajectory outputs of the frame windows (fbus_ekf_frames_fused_traj_dev / _frames_meas_fused_traj_dev) on the
bench's window shapes: B = 65 536 filters, one window = 30 camera frames behind 7 / 7 / 6 IMU samples, 4 marker slots; pose rows, left
pixels, stereo pixels.  Three variants of the same launch -- no outputs (the existing entry point), nominal rows only, all three outputs --
ALTERNATED in one process and timed with HIP events on the handle's stream; prints one JSON line per case with the median and the spread
(min / max) of each variant over the repetitions and the overheads against "none".
  python tools/time_window_traj.py [--batch 65536] [--reps 20] [--warmup 3]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fbus-ekf_amd"))

PATTERN, PATTERNS = (7, 7, 6), 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    from fbus_ekf import BatchedFilter, capi, synth
    dev = torch.device("cuda:0")
    B, M = args.batch, 4
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    kc = np.array(list(PATTERN) * PATTERNS, np.int32)
    F, Kt = len(kc), int(kc.sum())
    kcp = kc.ctypes.data_as(C.POINTER(C.c_int32))
    out_nom = torch.empty((F, B, 19), dtype=torch.float32, device=dev)
    out_pd = torch.empty((F, B, 18), dtype=torch.float32, device=dev)
    out_ap = torch.empty((F, B), dtype=torch.uint8, device=dev)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    variants = {"none": None, "nominal": (p(out_nom), None, None), "all": (p(out_nom), p(out_pd), p(out_ap))}

    prm = capi.default_params(capi.DIALECT_MATLAB)
    nom, rot, P, prev = synth.initial_state(0, B, list(prm.p0_diag), 18)
    acc, gyr = synth.imu_samples(0, B, 0, max(PATTERN), nom)
    w_acc = f32(np.concatenate([acc[:K] for K in kc]))
    w_gyr = f32(np.concatenate([gyr[:K] for K in kc]))
    w_dt = torch.full((Kt,), 0.005, dtype=torch.float32, device=dev)
    ids, pos, quat = synth.marker_frame(0, B, 0, M, nom, prm)
    w_ids = torch.from_numpy(ids).to(dev).unsqueeze(0).repeat(F, 1, 1).contiguous()
    w_pos = f32(pos).unsqueeze(0).repeat(F, 1, 1, 1).contiguous()
    w_quat = f32(quat).unsqueeze(0).repeat(F, 1, 1, 1).contiguous()

    size = 0.15
    pprm = capi.default_params(capi.DIALECT_MATLAB)
    pprm.marker_size = size
    pnom, prot, pids, left, right = synth.pixel_wall_scene(B, M, pprm, size, seed=9, stereo=True)
    pw_ids = torch.from_numpy(pids).to(dev).unsqueeze(0).repeat(F, 1, 1).contiguous()
    pw_left = f32(left).unsqueeze(0).repeat(F, 1, 1, 1).contiguous()
    pw_right = f32(right).unsqueeze(0).repeat(F, 1, 1, 1).contiguous()
    pacc, pgyr = synth.imu_samples(0, B, 0, max(PATTERN), pnom)
    pw_acc = f32(np.concatenate([pacc[:K] for K in kc]))
    pw_gyr = f32(np.concatenate([pgyr[:K] for K in kc]))

    cases = {
        "pose_m4": (prm, (nom, rot, P, prev), lambda flt, o: (
            flt._lib.fbus_ekf_frames_fused_dev(flt._h, F, kcp, p(w_acc), p(w_gyr), p(w_dt), 0, M, p(w_ids), p(w_pos), p(w_quat),
                                               capi.MODE_STACKED, None) if o is None else
            flt._lib.fbus_ekf_frames_fused_traj_dev(flt._h, F, kcp, p(w_acc), p(w_gyr), p(w_dt), 0, M, p(w_ids), p(w_pos), p(w_quat),
                                                    capi.MODE_STACKED, None, *o))),
    }
    for name, r in (("pixels_m4", None), ("pixels_m4_stereo", pw_right)):
        cases[name] = (pprm, (pnom, prot, None, np.zeros(B, np.int32)), lambda flt, o, r=r: (
            flt._lib.fbus_ekf_frames_meas_fused_dev(flt._h, F, kcp, p(pw_acc), p(pw_gyr), p(w_dt), 0, capi.MEAS_PIXELS, M, p(pw_ids),
                                                    p(pw_left), p(r), capi.VIS_REFRACTIVE, capi.MODE_STACKED, None) if o is None else
            flt._lib.fbus_ekf_frames_meas_fused_traj_dev(flt._h, F, kcp, p(pw_acc), p(pw_gyr), p(w_dt), 0, capi.MEAS_PIXELS, M, p(pw_ids),
                                                         p(pw_left), p(r), capi.VIS_REFRACTIVE, capi.MODE_STACKED, None, *o)))
    torch.cuda.synchronize()
    for name, (cprm, state, call) in cases.items():
        with BatchedFilter(B, cprm, order_streams=False) as flt:
            flt.set_state(*state)
            if state[2] is None:
                flt.reset_cov()
            flt.set_stream(torch.cuda.current_stream())
            st = torch.cuda.current_stream()
            times = {v: [] for v in variants}
            for rep in range(args.warmup + args.reps):
                for v, o in variants.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(st)
                    rc = call(flt, o)
                    e1.record(st)
                    if rc != 0:
                        raise RuntimeError(f"{name} {v}: {flt._lib.fbus_ekf_last_error(flt._h).decode()}")
                    torch.cuda.synchronize()
                    if rep >= args.warmup:
                        times[v].append(e0.elapsed_time(e1))
        med = {v: float(np.median(t)) for v, t in times.items()}
        print(json.dumps({"case": name, "B": B, "frames": F, "imu_samples": Kt, "reps": args.reps,
                          "ms_median": {v: round(m, 4) for v, m in med.items()},
                          "ms_min": {v: round(min(t), 4) for v, t in times.items()},
                          "ms_max": {v: round(max(t), 4) for v, t in times.items()},
                          "overhead_pct": {v: round(100 * (med[v] / med["none"] - 1), 2) for v in ("nominal", "all")}}), flush=True)


if __name__ == "__main__":
    main()
