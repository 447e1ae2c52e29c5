#!/usr/bin/env python3
"""What does every frame and window entry point run, and compute, in every handle state?  One line per cell of
    record type x covariance form x noise table x likelihood sums x set_team x size class (x a few environment knobs)
  x entry point (frame_fused, frames_fused, frame_meas_fused, frames_meas_fused; windows with and without trajectory rows, one-frame windows)
  x rows (pose nearest / stacked, pixels left / stereo, corners nearest / stacked) x M in {0, 1, 4} x K in {0, 3, 300}
with the return code, a sha256 over get_state(), applied() and the trajectory outputs, the launch counts of timing_read for every kernel
kind and the five route predicates of launch_info.  The handle is placed in each size class with set_policy_batch, derived from
launch_info(INFO_SIMDS).  Two libraries agree on every route and every result bit exactly when their outputs are equal line for line:
    FBUS_EKF_LIB=<parent build> python tools/route_matrix.py > a.txt ;  python tools/route_matrix.py > b.txt ;  diff a.txt b.txt
  python tools/route_matrix.py [--dtype 32|64] [--batch 128,100]
The handle states, inputs and calls are tests/route_cells.py's, shared with tests/test_routes_gpu.py (which asserts the signature and
window == frames on about a hundred of the cells)."""
import hashlib
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("fbus-ekf_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, sub))
import numpy as np
from fbus_ekf import capi
from route_cells import KC, KINDS, NEAREST, STACKED, Cfg, Data, make, one_frame, window

INFOS = ((capi.INFO_ROLES_PREDICT, 7), (capi.INFO_ROLES_MEAS, 4), (capi.INFO_TEAM_FRAMES, 0), (capi.INFO_MEAS_SPLIT, 4), (capi.INFO_NOISE_RESIDENT, 0))
ROWS = (("pose", NEAREST), ("pose", STACKED), ("left", STACKED), ("stereo", STACKED), ("corners", NEAREST), ("corners", STACKED))
SIZES = ("Q", "H", "H1", "R+1")
ENVS = ({"FBUS_TEAM_FRAME": "2"}, {"FBUS_TEAM_FRAME": "1"}, {"FBUS_MEAS_SPLIT": "0"}, {"FBUS_MEAS_SPLIT": "2"}, {"FBUS_NO_FRAME_MEAS": "1"})


def cfgs(dtypes):
    for dtype, joseph, noise, lik, team, size in itertools.product(dtypes, (0, 1), (0, 1), (0, 1), ((0, 0), (1, 1), (4, 4)), SIZES):
        yield Cfg(f"f{dtype} n18 joseph{joseph} noise{noise} lik{lik} team{team[0]}{team[1]} {size}", size, dtype, 18, 0, bool(joseph),
                  bool(noise), bool(lik), team)
    for dtype, size in itertools.product(dtypes, ("H", "H1")):                      # the N = 15 sample (the other dialect)
        yield Cfg(f"f{dtype} n15 cpp {size}", size, dtype, 15, 1)
    if 32 in dtypes:
        for env, noise, team, size in itertools.product(ENVS, (0, 1), ((0, 0), (1, 1)), SIZES):
            yield Cfg(f"f32 n18 {' '.join(k + '=' + v for k, v in env.items())} noise{noise} team{team[0]}{team[1]} {size}", size, noise=bool(noise),
                      team=team, env=env)


def calls():
    """(name, meas rows, call(f, d) -> trajectory outputs or None)"""
    for (kind, mode), M in itertools.product(ROWS, (0, 1, 4)):
        for K in (0, 3, 300):
            yield f"frame {kind} mode{mode} M{M} K{K}", kind != "pose", (lambda f, d, a=(kind, mode, M, K): one_frame(f, d, *a))
        for kc, rows in itertools.product((KC, (2,)), (False, True)):
            yield (f"frames {kind} mode{mode} M{M} kcount{kc} rows{int(rows)}", kind != "pose",
                   (lambda f, d, a=(kind, mode, M, kc, rows): window(f, d, *a)))


def digest(f, out):
    h = hashlib.sha256()
    for a in f.get_state() + (f.applied(),) + tuple(o.cpu().numpy() for o in (out or ())):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:24]


def main():
    arg = lambda name, default: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default
    dtypes = tuple(int(x) for x in arg("--dtype", "32,64").split(","))
    data, n = {}, 0
    for B in (int(x) for x in arg("--batch", "128,100").split(",")):
        for cfg in cfgs(dtypes):
            key = (cfg.dtype, cfg.nstate, cfg.dialect, B)
            if key not in data:
                data[key] = Data(*key)
            d = data[key]
            for meas in (False, True):
                with make(cfg, d, meas) as f:
                    info = " ".join(str(f.launch_info(w, a)) for w, a in INFOS)
                    for name, m, call in calls():
                        if m != meas:
                            continue
                        f.set_state(*(d.meas_state if meas else d.state))
                        f.timing_reset()
                        try:
                            out, rc = call(f, d), 0
                        except capi.FbusError as e:
                            out, rc = None, e.code
                        f.sync()
                        print(f"B{B} {cfg} | {name} | rc {rc} {digest(f, out)} | {' '.join(str(f.timing_read(k)[1]) for k in KINDS)} | {info}")
                        n += 1
    print(f"cells {n}")


if __name__ == "__main__":
    main()
