#!/usr/bin/env python3
"""Cost of the general row update beside the two built-in sensor updates on the same handle: B = 65 536 (records of 52 / 105 MB: a
cache + HBM rate, the Infinity Cache holds them between launches) and B = 1 048 576 (839 MB / 1.68 GB: the HBM rate), N = 18, fp32 and
fp64 records.  Four launches -- correct_rows_dev at m = 3 (the rows of fbus_ekf.rows.position_fix, formed once on the device from
get_state_dev) and at m = 1 (rows.range_to), correct_velocity_dev (the yardstick: the same record bytes, three rows on nine columns,
formed in the kernel) and correct_depth_dev (one row) -- ALTERNATED in one process and timed with device events on the handle's stream.
The whole measurement runs in TWO fresh processes, one after the other, each under its own time limit, so that the spread between
processes stands beside every median.  The bytes per filter are taken from the code (csrc/ekf_rows.hpp: every record chunk but the ones
holding only the carried rotation loaded and stored, res, H, applied: the velocity update's record bytes less the rotation chunks it
reads, plus m N + m input elements) and printed with the implied rate and the ratio to the velocity update.
Prints one JSON line per (process, dtype, B): median, min and max microseconds per launch.
  python tools/time_rows.py [--batches 65536 1048576] [--reps 40] [--warmup 5] [--processes 2] [--timeout 240]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fbus-ekf_amd"))


def record_chunks(dtype, N):
    """(chunks of a record, chunks a sensor update stores: all but the ones holding only the carried rotation, element size): the record
    layout of csrc/ekf_device.hpp (Rec<T, N>) restated"""
    es = 4 if dtype == 32 else 8
    epc = 16 // es
    nrec = 28 + N * (N + 1) // 2 + 1
    nch = (nrec + epc - 1) // epc
    ch_nom, ch_pq, ch_pqr = 28 // epc, (7 + epc - 1) // epc, 16 // epc
    return nch, ch_pq + (ch_nom - ch_pqr) + (nch - ch_nom), es


def rows_bytes_per_filter(dtype, N, m):
    """csrc/ekf_rows.hpp: the chunks it stores are the chunks it loads (it does not read R), + H + res + applied (the scalar variances
    are one load per wave)"""
    nch, stored, es = record_chunks(dtype, N)
    return 2 * stored * 16 + (m * N + m) * es + 1


def velocity_bytes_per_filter(dtype, N):
    """csrc/ekf_velocity.hpp: every chunk loaded (H is formed from R and v), + z + gyro + applied"""
    nch, stored, es = record_chunks(dtype, N)
    return (nch + stored) * 16 + 6 * es + 1


def measure(args, process):
    import torch
    from fbus_ekf import BatchedFilter, capi, rows, synth
    assert torch.cuda.is_available(), "time_rows.py measures on a GPU"
    dev = torch.device("cuda:0")
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    N = 18
    prm = capi.default_params(0)
    stream = torch.cuda.Stream(dev)
    axis, offset, dlever = np.array([0.12, -0.2, 1.0]), 0.4, np.array([0.11, -0.07, 0.05])
    a = np.array([1.0, -2.0, 3.0]) / np.sqrt(14.0)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    mount, lever = np.eye(3) + np.sin(0.3) * K + (1 - np.cos(0.3)) * (K @ K), np.array([0.21, -0.08, 0.12])
    beacon = np.array([4.0, -3.0, 1.5])
    for B in args.batches:
        nom, rot, _, prev = synth.initial_state(0, B, list(prm.p0_diag), N, with_cov=False)
        _, gyr = synth.imu_samples(0, B, 0, 1, nom)
        zd = synth.depth(0, B, 0, nom, rot, axis=axis, offset=offset, lever=dlever, noise=0.01)
        zv = synth.velocity(0, B, 0, nom, rot, gyr[0], mount=mount, lever=lever, noise=0.01)
        rng = np.random.default_rng(1)
        R = rot.reshape(B, 3, 3)
        zp = nom[:, 0:3] + R @ lever + rng.normal(0, 0.01, (B, 3))
        zr = np.linalg.norm(nom[:, 0:3] + R @ lever - beacon, axis=1) + rng.normal(0, 0.01, B)
        for dtype in args.dtypes:
            tt = torch.float32 if dtype == 32 else torch.float64
            up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev).to(tt)
            g_d, zd_d, zv_d, zp_d, zr_d = up(gyr[0]), up(zd), up(zv), up(zp), up(zr)
            dvar_d = torch.tensor([1e-4], dtype=torch.float64, device=dev)
            vvar_d = torch.tensor([1e-4, 4e-4, 2.5e-5], dtype=torch.float64, device=dev)
            torch.cuda.synchronize()
            with BatchedFilter(B, prm, device=0, dtype=dtype, nstate=N, stream=stream) as flt:
                flt.set_state(nom, rot, None, prev)
                flt.reset_cov()                       # the P0 diagonal, written on the device: no launch here branches on the covariance
                flt.set_depth_sensor(axis, offset, dlever)
                flt.set_velocity_sensor(mount, lever)
                with torch.cuda.stream(stream):
                    dn, dr = flt.get_state_dev()
                    res3, H3 = rows.position_fix(dn, dr, zp_d, lever, nstate=N)
                    res1, H1 = rows.range_to(dn, dr, zr_d, beacon, lever, nstate=N)
                    res3, H3, res1, H1 = (x.contiguous() for x in (res3, H3, res1, H1))
                stream.synchronize()
                lib, h = flt._lib, flt._h
                launches = {
                    "correct_rows_m3": lambda: lib.fbus_ekf_correct_rows_dev(h, 3, p(res3), p(H3), p(vvar_d), 0, None),
                    "correct_rows_m1": lambda: lib.fbus_ekf_correct_rows_dev(h, 1, p(res1), p(H1), p(dvar_d), 0, None),
                    "correct_velocity": lambda: lib.fbus_ekf_correct_velocity_dev(h, p(zv_d), p(g_d), p(vvar_d), 0, None),
                    "correct_depth": lambda: lib.fbus_ekf_correct_depth_dev(h, p(zd_d), p(dvar_d), 0, None),
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
            med = {k: float(np.median(v)) for k, v in times.items()}
            by = {"correct_rows_m3": rows_bytes_per_filter(dtype, N, 3), "correct_rows_m1": rows_bytes_per_filter(dtype, N, 1),
                  "correct_velocity": velocity_bytes_per_filter(dtype, N)}
            print(json.dumps({"process": process, "dtype": dtype, "B": B, "record_MB": round(bpf * B / 1e6, 1),
                              "rate_kind": "cache + HBM" if B <= 131072 else "HBM", "bytes_per_filter": by,
                              "bytes_rows_m3_over_velocity": round(by["correct_rows_m3"] / by["correct_velocity"], 3),
                              "TB_per_s": {k: round(by[k] * B / med[k] / 1e6, 3) for k in by},
                              "time_over_velocity": {k: round(med[k] / med["correct_velocity"], 3) for k in ("correct_rows_m3", "correct_rows_m1")},
                              "applied_share_last_launch": applied,
                              "us": {k: {"median": round(med[k], 2), "min": round(min(v), 2), "max": round(max(v), 2)}
                                     for k, v in times.items()}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[65536, 1048576])
    ap.add_argument("--dtypes", type=int, nargs="+", default=[32, 64])
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--processes", type=int, default=2)
    ap.add_argument("--timeout", type=float, default=240.0, help="time limit of each measuring process, seconds")
    ap.add_argument("--process", type=int, default=None, help="(internal) run the measurement here, as process number N")
    args = ap.parse_args()
    if args.process is not None:
        return measure(args, args.process)
    # this process never opens the GPU: each measurement is a fresh child under its own time limit, one at a time; a child that fails or
    # runs out of time ends the run
    for i in range(args.processes):
        cmd = [sys.executable, os.path.abspath(__file__), "--process", str(i), "--reps", str(args.reps), "--warmup", str(args.warmup),
               "--batches", *map(str, args.batches), "--dtypes", *map(str, args.dtypes)]
        try:
            rc = subprocess.run(cmd, timeout=args.timeout).returncode
        except subprocess.TimeoutExpired:
            print(f"process {i}: no result within {args.timeout:.0f} s", file=sys.stderr)
            sys.exit(124)
        if rc != 0:
            sys.exit(rc)


if __name__ == "__main__":
    main()
