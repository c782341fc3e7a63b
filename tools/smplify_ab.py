#!/usr/bin/env python3
"""SMPLify: the one-call loop (dposer_smplify_optimize) against fused=False (SMPLX + autograd + torch.optim.Adam), alternating on the same
device, with the reference's full schedule (100 camera + 5 x 100 body iterations) on the synthetic SMPL-X asset.

    python tools/smplify_ab.py [--batches 1,16,256,4096] [--reps 3] [--out smplify_ab.json] [--only-fused]

One warm-up call per path and batch, a device synchronise around every timed call; the median of --reps alternating pairs.  Writes one JSON.
--only-fused times the one call alone (for kernel traces)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


def build(B):
    from dposer_amd.body_model.smpl import SMPLX
    from dposer_amd.body_model.synthetic import make_synthetic_smplx_asset
    from dposer_amd.dataset.AMASS import Posenormalizer
    from dposer_amd.prior import DPoser
    from dposer_amd.tasks.smplify import SMPLify
    from gpu_common import make_model
    from helpers import load
    _, m, _ = make_model(27, precision="fp32")
    g = load("g10_normalizer")
    st = {k.split("/")[-1]: torch.tensor(g[k]) for k in g.files if k.startswith("stats/axis_normalize")}

    class Args:
        device = "cuda:0"
        sde_N = 500
        time_strategy = "3"

    nz = Posenormalizer(st, device="cuda:0", normalize=True, min_max=False, rot_rep="axis")
    prior = DPoser(batch_size=B, config_path="configs.subvp.amass_scorefc_continuous.get_config", args=Args(), model=m, normalizer=nz)
    return SMPLify(SMPLX(make_synthetic_smplx_asset(seed=0)).to("cuda:0"), batch_size=B, num_iters=100, args=Args(), pose_prior=prior)


def inputs(B):
    rs = np.random.RandomState(1)
    t = lambda a: torch.tensor(a, dtype=torch.float32, device="cuda:0")
    return (t(rs.standard_normal((B, 66)) * 0.1), t(rs.standard_normal((B, 10)) * 0.3),
            t(np.stack([rs.uniform(-.2, .2, B), rs.uniform(-.2, .2, B), rs.uniform(18, 26, B)], 1)), t(np.full((B, 2), 112.)),
            t(np.concatenate([112 + rs.standard_normal((B, 49, 2)) * 40, rs.uniform(.2, 1, (B, 49, 1))], 2)))


def timed(sm, x, fused):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sm(x[0], x[1], x[2], x[3], x[4].clone(), fused=fused)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,16,256,4096")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="smplify_ab.json")
    ap.add_argument("--only-fused", action="store_true")
    a = ap.parse_args()
    res = {"schedule": "100 camera + 5 x 100 body iterations", "asset": "synthetic SMPL-X (V = 10475)", "batches": {}}
    for B in [int(b) for b in a.batches.split(",")]:
        sm, x = build(B), inputs(B)
        paths = [True] if a.only_fused else [True, False]
        for f in paths:
            timed(sm, x, f)                                   # warm-up
        ts = {f: [] for f in paths}
        for _ in range(a.reps):
            for f in paths:
                ts[f].append(timed(sm, x, f))
        r = {"one_call_s": float(np.median(ts[True]))}
        if not a.only_fused:
            r["step_by_step_s"] = float(np.median(ts[False]))
            r["speedup"] = r["step_by_step_s"] / r["one_call_s"]
        res["batches"][str(B)] = r
        print(B, r, flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
