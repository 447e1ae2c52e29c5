#!/usr/bin/env python3
"""Cost of fbus_ekf_sample_dev beside two launches that are known, on one handle: 65 536 and 1 048 576 filters, N = 18, fp32 and fp64
records.  Five launches -- sample_dev with S = 1 (state and drawn), with S = 2N + 1 = 37 (the sigma points), with S = 37 and drawn only
(the stream and the factorisation without the loop: what the 37 rows cost is the difference); nees_dev with all three outputs;
predict_dev (one sample) -- ALTERNATED in one process and timed with device events on the handle's stream.  sample reads the whole record
once, as nees does, and factorises it in the same order; per draw it reads N and writes 19 doubles per filter.  The expectation to hold the
figures against: S = 1 costs about what nees_dev with all outputs costs.  predict moves the state a little every repetition; no launch
here depends on the values it reads.
Every (batch, dtype) case is a process of its own under its own time limit, and the cases are run in turn `--rounds` times, so that a
drift of the machine shows as a difference between the rounds.  The states of the larger batch are those of the first 65 536 filters,
repeated on the device; the 37 rows of xi are the sigma points, the same for every filter.
Prints one JSON line per case and round: median, min and max microseconds per launch, and the record bytes.
  python tools/time_sample.py [--batches 65536 1048576] [--rounds 2] [--reps 30] [--warmup 5] [--limit 240]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fbus-ekf_amd"))
BASE = 65536


def child(B, dtype, reps, warmup):
    import torch
    from fbus_ekf import BatchedFilter, capi, consistency, synth
    assert torch.cuda.is_available(), "time_sample.py measures on a GPU"
    dev = torch.device("cuda:0")
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    N = 18
    SS = 2 * N + 1
    tt = torch.float32 if dtype == 32 else torch.float64
    prm = capi.default_params(0)
    nb = min(B, BASE)
    assert B % nb == 0
    nom, rot, P, prev = synth.initial_state(0, nb, list(prm.p0_diag), N, mixed_cov=True)
    acc, gyr = synth.imu_samples(0, nb, 0, 1, nom)
    rep = lambda t: t.repeat((B // nb,) + (1,) * (t.dim() - 1)).contiguous()
    up = lambda a, t=None: rep(torch.from_numpy(np.ascontiguousarray(a)).to(dev).to(t or tt))
    n_d, r_d, P_d, pv_d = up(nom), up(rot), up(P), up(np.asarray(prev, np.int32), torch.int32)
    a_d, g_d = up(acc[0]), up(gyr[0])
    dt_d = torch.full((1,), 0.005, dtype=tt, device=dev)
    truth = up(nom, torch.float64)
    truth[:, 0:6] += 0.01
    pts, _ = consistency.sigma_points(N)
    xi = torch.from_numpy(pts).to(dev)[:, None, :].expand(SS, B, N).contiguous()
    xi1 = torch.randn((1, B, N), dtype=torch.float64, device=dev)
    o_state = torch.empty((SS, B, 19), dtype=torch.float64, device=dev)
    o_drawn = torch.empty(B, dtype=torch.uint8, device=dev)
    o_nees = torch.empty((B, capi.NEES_COLS), dtype=torch.float64, device=dev)
    o_err = torch.empty((B, N), dtype=torch.float64, device=dev)
    o_lnp = torch.empty(B, dtype=torch.float64, device=dev)
    stream = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    with BatchedFilter(B, prm, device=0, dtype=dtype, nstate=N, stream=stream) as flt:
        flt.order_streams = False
        lib, h = flt._lib, flt._h
        assert lib.fbus_ekf_set_state_dev(h, p(n_d), p(r_d), p(P_d), p(pv_d)) == 0
        launches = {
            "sample_1": lambda: lib.fbus_ekf_sample_dev(h, 1, p(xi1), None, p(o_state), p(o_drawn)),
            "sample_37": lambda: lib.fbus_ekf_sample_dev(h, SS, p(xi), None, p(o_state), p(o_drawn)),
            "drawn_only": lambda: lib.fbus_ekf_sample_dev(h, SS, p(xi), None, None, p(o_drawn)),
            "nees_all": lambda: lib.fbus_ekf_nees_dev(h, p(truth), None, p(o_nees), p(o_err), p(o_lnp)),
            "predict": lambda: lib.fbus_ekf_predict_dev(h, p(a_d), p(g_d), p(dt_d), 0),
        }
        times = {k: [] for k in launches}
        for r in range(warmup + reps):
            for k, fn in launches.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                assert fn() == 0, (k, lib.fbus_ekf_last_error(h))
                e1.record(stream)
                e1.synchronize()
                if r >= warmup:
                    times[k].append(e0.elapsed_time(e1) * 1e3)
        flt.sync()
        drawn = float(o_drawn.float().mean())
        _, bpf, _ = flt.records()
    med = {k: float(np.median(v)) for k, v in times.items()}
    print(json.dumps({"B": B, "dtype": dtype, "record_MB": round(bpf * B / 1e6, 1), "drawn": round(drawn, 4),
                      "sample_1_over_nees_all": round(med["sample_1"] / med["nees_all"], 3),
                      "sample_1_over_predict": round(med["sample_1"] / med["predict"], 3),
                      "us_per_row_37": round((med["sample_37"] - med["drawn_only"]) / SS, 2),
                      "rows_37_MB": round(SS * B * (19 + N) * 8 / 1e6, 1),
                      "us": {k: {"median": round(med[k], 2), "min": round(min(v), 2), "max": round(max(v), 2)} for k, v in times.items()}}),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[BASE, 16 * BASE])
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--limit", type=float, default=240.0, help="seconds a case may take")
    ap.add_argument("--child", type=int, nargs=2, metavar=("B", "DTYPE"))
    args = ap.parse_args()
    if args.child:
        return child(args.child[0], args.child[1], args.reps, args.warmup)
    for rnd in range(args.rounds):
        for B in args.batches:
            for dtype in (32, 64):
                cmd = [sys.executable, os.path.abspath(__file__), "--child", str(B), str(dtype), "--reps", str(args.reps),
                       "--warmup", str(args.warmup)]
                try:
                    rc = subprocess.run(cmd, timeout=args.limit).returncode
                except subprocess.TimeoutExpired:
                    rc = 124
                if rc != 0:             # a case that failed or ran into its limit ends the run: nothing more is started on the device
                    print(json.dumps({"B": B, "dtype": dtype, "round": rnd, "failed": rc}), flush=True)
                    return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
