#!/usr/bin/env python3
"""Cost of the depth update beside the stacked pose update and the per-call predict on the same handle: B = 65 536 (records of 52 / 105 MB:
a cache + HBM rate, the Infinity Cache holds them between launches) and B = 1 048 576 (839 MB / 1.68 GB: the HBM rate), N = 18, fp32 and
fp64 records.  Three launches -- correct_depth_dev (scalar variance, no skip), correct_dev (stacked, M = 1: the yardstick, it moves the
same record and applies six rank-1 passes where the depth update applies one) and predict_dev -- ALTERNATED in one process and timed with
device events on the handle's stream.  The bytes per filter the depth kernel moves are taken from the code (csrc/ekf_depth.hpp: every
record chunk loaded, every chunk but the ones holding only the carried rotation stored, z, applied) and printed with the implied rate.
Prints one JSON line per (dtype, B): median, min and max microseconds per launch.
  python tools/time_depth.py [--batches 65536 1048576] [--reps 40] [--warmup 5]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fbus-ekf_amd"))


def depth_bytes_per_filter(dtype, N):
    """loads + stores of correct_depth_kernel per filter: the record layout of csrc/ekf_device.hpp (Rec<T, N>) restated"""
    es = 4 if dtype == 32 else 8
    epc = 16 // es
    nrec = 28 + N * (N + 1) // 2 + 1
    nch = (nrec + epc - 1) // epc
    ch_nom, ch_pq, ch_pqr = 28 // epc, (7 + epc - 1) // epc, 16 // epc
    loaded = nch
    stored = ch_pq + (ch_nom - ch_pqr) + (nch - ch_nom)
    return (loaded + stored) * 16 + es + 1, loaded, stored          # + z + applied (the scalar variance is one load per wave)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[65536, 1048576])
    ap.add_argument("--dtypes", type=int, nargs="+", default=[32, 64])
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import torch
    from fbus_ekf import BatchedFilter, capi, synth
    assert torch.cuda.is_available(), "time_depth.py measures on a GPU"
    dev = torch.device("cuda:0")
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    N = 18
    prm = capi.default_params(0)
    stream = torch.cuda.Stream(dev)
    axis, offset, lever = np.array([0.12, -0.2, 1.0]), 0.4, np.array([0.11, -0.07, 0.05])
    for B in args.batches:
        nom, rot, _, prev = synth.initial_state(0, B, list(prm.p0_diag), N, with_cov=False)
        acc, gyr = synth.imu_samples(0, B, 0, 1, nom)
        ids, pos, quat = synth.marker_frame(0, B, 0, 1, nom, prm)
        z = synth.depth(0, B, 0, nom, rot, axis=axis, offset=offset, lever=lever, noise=0.01)
        for dtype in args.dtypes:
            tt = torch.float32 if dtype == 32 else torch.float64
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev).to(tt)
            a_d, g_d, pos_d, quat_d, z_d = up(acc[0]), up(gyr[0]), up(pos), up(quat), up(z)
            dt_d = up(np.array([0.005]))
            ids_d = torch.from_numpy(np.ascontiguousarray(ids, np.int32)).to(dev)
            var_d = torch.tensor([1e-4], dtype=torch.float64, device=dev)
            torch.cuda.synchronize()
            with BatchedFilter(B, prm, device=0, dtype=dtype, nstate=N, stream=stream) as flt:
                flt.set_state(nom, rot, None, prev)
                flt.reset_cov()                       # the P0 diagonal, written on the device: no launch here branches on the covariance
                flt.set_depth_sensor(axis, offset, lever)
                lib, h = flt._lib, flt._h
                launches = {
                    "correct_depth": lambda: lib.fbus_ekf_correct_depth_dev(h, p(z_d), p(var_d), 0, None),
                    "correct_stacked_M1": lambda: lib.fbus_ekf_correct_dev(h, 1, p(ids_d), p(pos_d), p(quat_d), capi.MODE_STACKED, None),
                    "predict": lambda: lib.fbus_ekf_predict_dev(h, p(a_d), p(g_d), p(dt_d), 0),
                }
                times = {k: [] for k in launches}
                for rep in range(args.warmup + args.reps):
                    for k, fn in launches.items():
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(stream)
                        assert fn() == 0
                        e1.record(stream)
                        e1.synchronize()
                        if rep >= args.warmup:
                            times[k].append(e0.elapsed_time(e1) * 1e3)
                applied = float(flt.applied().mean())
                _, bpf, _ = flt.records()
            per, loaded, stored = depth_bytes_per_filter(dtype, N)
            med = float(np.median(times["correct_depth"]))
            print(json.dumps({"dtype": dtype, "B": B, "record_MB": round(bpf * B / 1e6, 1), "rate_kind": "cache + HBM" if B <= 131072 else "HBM",
                              "depth_bytes_per_filter": per, "chunks_loaded": loaded, "chunks_stored": stored,
                              "depth_TB_per_s": round(per * B / med / 1e6, 3), "applied_share_last_launch": applied,
                              "us": {k: {"median": round(float(np.median(v)), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
                                     for k, v in times.items()}}), flush=True)


if __name__ == "__main__":
    main()
