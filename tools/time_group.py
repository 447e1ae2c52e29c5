#!/usr/bin/env python3
"""Cost of the hypothesis-group kernels beside fbus_ekf_snapshot_dev on the same handle: B = 65 536 filters, N = 18, fp32 and fp64 records,
G = 4, 9 (a 3 x 3 grid: 65 536 is no multiple of 9, so that case runs 65 529 filters) and 64.  Five launches -- snapshot_dev (nominal +
pdiag + applied), group_fuse_dev with the full P, group_fuse_dev with pdiag only, group_mix_dev (imm_transition(G, 0.9)),
group_collapse_dev (src = best) -- ALTERNATED in one process and timed with device events on the handle's stream; the records are the
same before every launch (behind mix and behind collapse, which write them, the state is restored from a device copy, outside the timed
span).  The yardstick is the record read itself: bytes per filter x B, printed with each case; for mix it is collapse, which like it
reads and writes every record.
Prints one JSON line per (dtype, G): median, min and max microseconds per launch.
  python tools/time_group.py [--batch 65536] [--reps 40] [--warmup 5]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fbus-ekf_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--groups", type=int, nargs="+", default=[4, 9, 64])
    args = ap.parse_args()
    import torch
    from fbus_ekf import BatchedFilter, capi, noise, synth
    assert torch.cuda.is_available(), "time_group.py measures on a GPU"
    dev = torch.device("cuda:0")
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    N = 18
    prm = capi.default_params(0)
    stream = torch.cuda.Stream(dev)
    nom0, rot0, P0, prev0 = synth.initial_state(0, args.batch, list(prm.p0_diag), N, mixed_cov=True)
    for dtype in (32, 64):
        tt = torch.float32 if dtype == 32 else torch.float64
        for G in args.groups:
            B = args.batch // G * G
            NG = B // G
            nom, rot, P, prev = nom0[:B], rot0[:B], P0[:B], prev0[:B]
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev).to(tt)
            n_d, r_d, P_d = up(nom), up(rot), up(P)
            pv_d = torch.from_numpy(np.ascontiguousarray(prev, np.int32)).to(dev)
            logw = torch.from_numpy(np.random.default_rng(G).uniform(-4.0, 0.0, B)).to(dev)
            trans = torch.from_numpy(noise.imm_transition(G, 0.9)).to(dev)
            weight, logc = (torch.empty(B, dtype=torch.float64, device=dev) for _ in range(2))
            best = torch.empty(NG, dtype=torch.int32, device=dev)
            f_nom, f_P, f_pd = (torch.empty(s, dtype=tt, device=dev) for s in ((NG, 19), (NG, N, N), (NG, N)))
            s_nom, s_pd = torch.empty((B, 19), dtype=tt, device=dev), torch.empty((B, N), dtype=tt, device=dev)
            s_app = torch.empty(B, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            with BatchedFilter(B, prm, device=0, dtype=dtype, nstate=N, stream=stream) as flt:
                lib, h = flt._lib, flt._h
                restore = lambda: lib.fbus_ekf_set_state_dev(h, p(n_d), p(r_d), p(P_d), p(pv_d))
                assert restore() == 0
                launches = {
                    "snapshot": lambda: lib.fbus_ekf_snapshot_dev(h, p(s_nom), p(s_pd), p(s_app)),
                    "fuse_full": lambda: lib.fbus_ekf_group_fuse_dev(h, G, p(logw), p(weight), p(best), p(f_nom), p(f_P), p(f_pd)),
                    "fuse_pdiag": lambda: lib.fbus_ekf_group_fuse_dev(h, G, p(logw), p(weight), p(best), p(f_nom), None, p(f_pd)),
                    "mix": lambda: lib.fbus_ekf_group_mix_dev(h, G, p(logw), p(trans), p(weight), p(logc)),
                    "collapse": lambda: lib.fbus_ekf_group_collapse_dev(h, G, p(best)),
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
                        if k in ("mix", "collapse"):
                            assert restore() == 0
                            flt.sync()
                _, bpf, total = flt.records()
            print(json.dumps({"dtype": dtype, "G": G, "B": B, "record_MB": round(bpf * B / 1e6, 1),
                              "us": {k: {"median": round(float(np.median(v)), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
                                     for k, v in times.items()}}), flush=True)


if __name__ == "__main__":
    main()
