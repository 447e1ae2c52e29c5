#!/usr/bin/env python3
"""Cost of the velocity update beside its two yardsticks on the same handle: B = 65 536 (records of 52 / 105 MB: a cache + HBM rate, the
Infinity Cache holds them between launches) and B = 1 048 576 (839 MB / 1.68 GB: the HBM rate), N = 18, fp32 and fp64 records.  Three
launches -- correct_velocity_dev (scalar variance triple, gyro given, no skip), correct_depth_dev (it moves the same record bytes and
applies one rank-1 pass where the velocity update applies three) and correct_dev (stacked, M = 1: the same record and seven rows) --
ALTERNATED in one process and timed with device events on the handle's stream.  The whole measurement runs in TWO fresh processes, one
after the other, so that the spread between processes stands beside every median.  The bytes per filter the velocity kernel moves are
taken from the code (csrc/ekf_velocity.hpp: every record chunk loaded, every chunk but the ones holding only the carried rotation stored,
z, gyro, applied) and printed with the implied rate.
Prints one JSON line per (process, dtype, B): median, min and max microseconds per launch.
  python tools/time_velocity.py [--batches 65536 1048576] [--reps 40] [--warmup 5] [--processes 2]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fbus-ekf_amd"))


def velocity_bytes_per_filter(dtype, N):
    """loads + stores of correct_velocity_kernel per filter: the record layout of csrc/ekf_device.hpp (Rec<T, N>) restated"""
    es = 4 if dtype == 32 else 8
    epc = 16 // es
    nrec = 28 + N * (N + 1) // 2 + 1
    nch = (nrec + epc - 1) // epc
    ch_nom, ch_pq, ch_pqr = 28 // epc, (7 + epc - 1) // epc, 16 // epc
    loaded = nch
    stored = ch_pq + (ch_nom - ch_pqr) + (nch - ch_nom)
    return (loaded + stored) * 16 + 6 * es + 1, loaded, stored      # + z + gyro + applied (the scalar variances are one load per wave)


def measure(args, process):
    import torch
    from fbus_ekf import BatchedFilter, capi, synth
    assert torch.cuda.is_available(), "time_velocity.py measures on a GPU"
    dev = torch.device("cuda:0")
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    N = 18
    prm = capi.default_params(0)
    stream = torch.cuda.Stream(dev)
    axis, offset, dlever = np.array([0.12, -0.2, 1.0]), 0.4, np.array([0.11, -0.07, 0.05])
    a = np.array([1.0, -2.0, 3.0]) / np.sqrt(14.0)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    mount, lever = np.eye(3) + np.sin(0.3) * K + (1 - np.cos(0.3)) * (K @ K), np.array([0.21, -0.08, 0.12])
    for B in args.batches:
        nom, rot, _, prev = synth.initial_state(0, B, list(prm.p0_diag), N, with_cov=False)
        _, gyr = synth.imu_samples(0, B, 0, 1, nom)
        ids, pos, quat = synth.marker_frame(0, B, 0, 1, nom, prm)
        zd = synth.depth(0, B, 0, nom, rot, axis=axis, offset=offset, lever=dlever, noise=0.01)
        zv = synth.velocity(0, B, 0, nom, rot, gyr[0], mount=mount, lever=lever, noise=0.01)
        for dtype in args.dtypes:
            tt = torch.float32 if dtype == 32 else torch.float64
            up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev).to(tt)
            g_d, pos_d, quat_d, zd_d, zv_d = up(gyr[0]), up(pos), up(quat), up(zd), up(zv)
            ids_d = torch.from_numpy(np.ascontiguousarray(ids, np.int32)).to(dev)
            dvar_d = torch.tensor([1e-4], dtype=torch.float64, device=dev)
            vvar_d = torch.tensor([1e-4, 4e-4, 2.5e-5], dtype=torch.float64, device=dev)
            torch.cuda.synchronize()
            with BatchedFilter(B, prm, device=0, dtype=dtype, nstate=N, stream=stream) as flt:
                flt.set_state(nom, rot, None, prev)
                flt.reset_cov()                       # the P0 diagonal, written on the device: no launch here branches on the covariance
                flt.set_depth_sensor(axis, offset, dlever)
                flt.set_velocity_sensor(mount, lever)
                lib, h = flt._lib, flt._h
                launches = {
                    "correct_velocity": lambda: lib.fbus_ekf_correct_velocity_dev(h, p(zv_d), p(g_d), p(vvar_d), 0, None),
                    "correct_depth": lambda: lib.fbus_ekf_correct_depth_dev(h, p(zd_d), p(dvar_d), 0, None),
                    "correct_stacked_M1": lambda: lib.fbus_ekf_correct_dev(h, 1, p(ids_d), p(pos_d), p(quat_d), capi.MODE_STACKED, None),
                }
                times = {k: [] for k in launches}
                applied = {}
                for rep in range(args.warmup + args.reps):
                    for k, fn in launches.items():
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(stream)
                        assert fn() == 0
                        e1.record(stream)
                        e1.synchronize()
                        if rep >= args.warmup:
                            times[k].append(e0.elapsed_time(e1) * 1e3)
                        if rep == args.warmup + args.reps - 1:
                            applied[k] = float(flt.applied().mean())
                _, bpf, _ = flt.records()
            per, loaded, stored = velocity_bytes_per_filter(dtype, N)
            med = float(np.median(times["correct_velocity"]))
            print(json.dumps({"process": process, "dtype": dtype, "B": B, "record_MB": round(bpf * B / 1e6, 1),
                              "rate_kind": "cache + HBM" if B <= 131072 else "HBM", "velocity_bytes_per_filter": per,
                              "chunks_loaded": loaded, "chunks_stored": stored, "velocity_TB_per_s": round(per * B / med / 1e6, 3),
                              "applied_share_last_launch": applied,
                              "us": {k: {"median": round(float(np.median(v)), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
                                     for k, v in times.items()}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[65536, 1048576])
    ap.add_argument("--dtypes", type=int, nargs="+", default=[32, 64])
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--processes", type=int, default=2)
    ap.add_argument("--process", type=int, default=None, help="(internal) run the measurement here, as process number N")
    args = ap.parse_args()
    if args.process is not None:
        return measure(args, args.process)
    # this process never opens the GPU: each measurement is a fresh child, one at a time
    for i in range(args.processes):
        cmd = [sys.executable, os.path.abspath(__file__), "--process", str(i), "--reps", str(args.reps), "--warmup", str(args.warmup),
               "--batches", *map(str, args.batches), "--dtypes", *map(str, args.dtypes)]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            sys.exit(rc)


if __name__ == "__main__":
    main()
