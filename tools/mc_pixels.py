#!/usr/bin/env python3
"""A Monte-Carlo consistency run of the pixel update that never leaves the device: for every filter a truth is DRAWN from its own
N(estimate, P) (BatchedFilter.sample), a second handle is set to the truths and projects them (consistency.observe: project_markers plus
N(0, r_pix) per coordinate), the first handle folds those pixels (correct_pixels) and is judged against the truths (nees).  Under a
consistent update the posterior NEES columns are chi-square again; consistency.summary prints the column means against their intervals.
Informational, not a test: with the prior of synth.initial_state (1 cm, 10 mrad) the second-order term of the projection is as large as
the posterior's own sigma, and ONE linearised update is over-confident in p and theta; --prior-scale 0.01 is the regime in which the
linearisation holds.
  python tools/mc_pixels.py [--batch 16384] [--dtype 32] [--cameras 2] [--seed 1] [--prior-scale 1.0]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fbus-ekf_amd"))


def rot_of(q):
    """(B, 9) rotation matrices of unit quaternions (B, 4) wxyz, float64, on the device (the formula of BatchedFilter.perturb)"""
    import torch
    w, x, y, z = q.unbind(1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--dtype", type=int, default=32, choices=(32, 64))
    ap.add_argument("--cameras", type=int, default=2, choices=(1, 2))
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--prior-scale", type=float, default=1.0, help="factor on the prior covariance (0.01: a tenth of every sigma)")
    args = ap.parse_args()
    import torch
    from fbus_ekf import BatchedFilter, capi, consistency, synth
    assert torch.cuda.is_available(), "mc_pixels.py runs on a GPU"
    dev = torch.device("cuda:0")
    B, N = args.batch, 18
    tt = torch.float32 if args.dtype == 32 else torch.float64
    prm = capi.default_params(0)
    prm.marker_size = 0.28
    nom, rot, ids, _, _ = synth.pixel_wall_scene(B, 4, prm, 0.28, stereo=True)
    _, _, P, prev = synth.initial_state(0, B, list(prm.p0_diag), N, mixed_cov=True)
    P = P * args.prior_scale
    gen =torch.Generator(device=dev)
    gen.manual_seed(args.seed)
    d_ids = torch.from_numpy(np.ascontiguousarray(ids, np.int32)).to(dev)
    with BatchedFilter(B, prm, device=0, dtype=args.dtype, nstate=N) as est, BatchedFilter(B, prm, device=0, dtype=args.dtype, nstate=N) as tru:
        est.set_state(nom, rot, P, prev)
        tru.set_state(nom, rot, P, prev)
        state, xi = consistency.draw(est, 1, gen)                                # truths ~ N(estimate, P)
        truth = state[0]
        prior = est.nees(truth)
        t_nom = truth.to(tt).contiguous()
        q = t_nom[:, 6:10].to(torch.float64)
        t_rot = rot_of(q / q.norm(dim=1, keepdim=True)).to(tt).contiguous()
        tru.set_state(t_nom, t_rot, None, None)
        ids_seen, left, right = consistency.observe(tru, d_ids, float(np.sqrt(prm.r_pix)), gen, args.cameras)
        est.correct_pixels(ids_seen.contiguous(), left.contiguous(), None if right is None else right.contiguous())
        post = est.nees(truth)
        seen = float((ids_seen >= 0).float().sum(dim=1).mean())
        est.sync()
        out = {"B": B, "dtype": args.dtype, "cameras": args.cameras, "prior_scale": args.prior_scale, "markers_seen_per_filter": round(seen, 2),
               "prior": consistency.summary(prior.cpu().numpy(), N), "posterior": consistency.summary(post.cpu().numpy(), N)}
    for k in ("prior", "posterior"):
        print(k, json.dumps({c: {"mean": round(v["mean"], 4), "lo": round(v["lo"], 4), "hi": round(v["hi"], 4), "inside": v["inside"]}
                             for c, v in out[k].items()}))
    print(json.dumps({k: out[k] for k in ("B", "dtype", "cameras", "prior_scale", "markers_seen_per_filter")}))


if __name__ == "__main__":
    main()
