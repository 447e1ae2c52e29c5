#!/usr/bin/env python3
"""Cost of the innovation log-likelihood sums (fbus_ekf_loglik_enable) on the per-call pose / pixel / corner updates at B = 65 536
filters, N = 18, fp32 and fp64 records: three variants of the same update -- the twin (fbus_ekf_correct_dev / _pixels_dev / _corners_dev),
the _nis_dev entry point with accumulation off (the kernels of the commit before the sums: the same instruction streams, tools/isa_diff.py)
and the same _nis_dev call with accumulation on (the tabled kernel with the sums, the handle's own noise row in the table) -- ALTERNATED
in one process and timed with HIP events on the handle's stream; the state is reset from a device copy before every launch.  Cases: pose
stacked M = 4, pixels left M = 4 and 16, pixels stereo M = 4 and 16, corners (3-D) stacked M = 4.
Prints one JSON line per case and record type: median and min / max per variant, overheads against the twin and of the sums against _nis.
  python tools/time_loglik.py [--batch 65536] [--reps 60] [--warmup 3]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fbus-ekf_amd"))


def run(args, dtype):
    import torch
    from fbus_ekf import BatchedFilter, capi, synth
    dev = torch.device("cuda:0")
    B = args.batch
    prm = capi.default_params(0)
    nom, rot, P, prev = synth.initial_state(0, B, list(prm.p0_diag), 18, mixed_cov=True)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    dof = torch.empty(B, dtype=torch.int32, device=dev)
    cases = [("pose_stacked_m4", "pose", 4, False), ("pixels_left_m4", "pixels", 4, False), ("pixels_left_m16", "pixels", 16, False),
             ("pixels_stereo_m4", "pixels", 4, True), ("pixels_stereo_m16", "pixels", 16, True), ("corners_stacked_m4", "corners", 4, False)]
    npt = np.float32 if dtype == 32 else np.float64
    f32 = lambda a, npt=npt: torch.from_numpy(np.ascontiguousarray(a, npt)).to(dev)        # (the record type's arrays)
    nis = torch.empty(B, dtype=torch.float32 if dtype == 32 else torch.float64, device=dev)
    with BatchedFilter(B, prm, device=0, dtype=dtype, nstate=18) as flt:
        flt.order_streams = False
        flt.set_state(nom, rot, P, prev)
        lib, h = flt._lib, flt._h
        n_d, r_d, P_d, pv_d = f32(nom), f32(rot), f32(P), torch.from_numpy(np.ascontiguousarray(prev, np.int32)).to(dev)
        for name, kind, M, stereo in cases:
            ids = np.broadcast_to(np.resize(synth.marker_table(prm)[0], M), (B, M))     # every slot a map marker (repeats past the map)
            if kind == "pose":
                ids, pos, quat = synth.marker_frame(0, B, 0, M, nom, prm)
                dp, dq = f32(pos), f32(quat)
            rng = np.random.default_rng(1)
            left = f32(rng.uniform(-0.3, 0.3, (B, M, 12 if kind == "corners" else 8)))
            right = f32(rng.uniform(-0.3, 0.3, (B, M, 8))) if stereo else None
            di = torch.from_numpy(np.ascontiguousarray(ids, np.int32)).to(dev)

            def twin():
                if kind == "pose":
                    return lib.fbus_ekf_correct_dev(h, M, p(di), p(dp), p(dq), capi.MODE_STACKED, None)
                if kind == "pixels":
                    return lib.fbus_ekf_correct_pixels_dev(h, M, p(di), p(left), p(right), None)
                return lib.fbus_ekf_correct_corners_dev(h, M, p(di), p(left), None, capi.VIS_CORNERS3D, capi.MODE_STACKED, None)

            def with_nis():
                if kind == "pose":
                    return lib.fbus_ekf_correct_nis_dev(h, M, p(di), p(dp), p(dq), capi.MODE_STACKED, None, p(nis), p(dof))
                if kind == "pixels":
                    return lib.fbus_ekf_correct_pixels_nis_dev(h, M, p(di), p(left), p(right), None, p(nis), p(dof))
                return lib.fbus_ekf_correct_corners_nis_dev(h, M, p(di), p(left), None, capi.VIS_CORNERS3D, capi.MODE_STACKED, None,
                                                            p(nis), p(dof))
            variants = {"twin": (twin, False), "nis": (with_nis, False), "nis_loglik": (with_nis, True)}
            times = {k: [] for k in variants}
            for rep in range(args.warmup + args.reps):
                for k, (fn, lik) in variants.items():
                    flt.loglik_enable(lik)
                    rc = lib.fbus_ekf_set_state_dev(h, p(n_d), p(r_d), p(P_d), p(pv_d))
                    assert rc == 0
                    flt.timing_enable(True)
                    flt.timing_reset()
                    assert fn() == 0
                    flt.sync()
                    ms = flt.timing_read(capi.KERNEL_CORRECT if kind == "pose" else capi.KERNEL_CORRECT_CORNERS)[0]
                    flt.timing_enable(False)
                    if rep >= args.warmup:
                        times[k].append(ms * 1e3)
            med = {k: float(np.median(v)) for k, v in times.items()}
            print(json.dumps({"case": name, "dtype": dtype, "B": B, "us": {k: {"median": round(med[k], 2), "min": round(min(v), 2), "max": round(max(v), 2)}
                                                         for k, v in times.items()},
                              "overhead_pct": {k: round(100 * (med[k] / med["twin"] - 1), 2) for k in ("nis", "nis_loglik")},
                              "loglik_vs_nis_pct": round(100 * (med["nis_loglik"] / med["nis"] - 1), 2)}),
                  flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    for dtype in (32, 64):
        run(args, dtype)


if __name__ == "__main__":
    main()
