#!/usr/bin/env python3
"""Probability-flow sampler (pc_sampler with probability_flow = True, EM predictor, corrector 'none', N steps): the one call
(dposer_pf_sampler, fused-epilogue form: no trajectory) against the generic loop the same pc_sampler ran before it existed (per step one
HIP score evaluation + torch elementwise ops), alternating on the same device from the same latents.

    python tools/pf_time.py [--batches 6,300,4096,65536] [--precs bf16,bf16x3] [--n 1000] [--reps 3] [--out pf_time.json]
    python tools/pf_time.py --only fused|generic --batches 300 --precs bf16 --reps 1      (one leg alone, for kernel traces)

Device events around every timed call, one warm-up call per leg; the median of --reps alternating pairs.  The outputs of the two legs of
the last pair are compared (max abs and relative L2 difference).  Writes one JSON."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


def sampler(cfg, B, N):
    from dposer_amd.algorithms.advanced import sampling, sde_lib
    cfg.sampling.probability_flow = True
    cfg.sampling.predictor = "euler_maruyama"
    cfg.sampling.corrector = "none"
    return sampling.get_sampling_fn(cfg, sde_lib.subVPSDE(0.1, 20.0, N), (B, 63), lambda v: v, 1e-5, device="cuda:0")


def run(fn, m, z, leg):
    """One pc_sampler call; leg 'generic' makes the fused entry unavailable, which is what pc_sampler did under probability flow before."""
    from dposer_amd.algorithms.advanced import sampling
    real = sampling.fused_em_supported
    if leg == "generic":
        sampling.fused_em_supported = lambda *a, **k: False
    try:
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        _, x = fn(m, z=z, traj_stride=0)
        end.record()
        torch.cuda.synchronize()
    finally:
        sampling.fused_em_supported = real
    return start.elapsed_time(end), x


def main():
    from gpu_common import make_model
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="6,300,4096,65536")
    ap.add_argument("--precs", default="bf16,bf16x3")
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", choices=["fused", "generic"], default=None)
    ap.add_argument("--out", default="pf_time.json")
    a = ap.parse_args()
    legs = [a.only] if a.only else ["fused", "generic"]
    res = {"N": a.n, "sde": "subVPSDE(0.1, 20, N)", "eps": 1e-5, "network": "ScoreModelFC H = 1024, 2 blocks, D = 63", "runs": []}
    for prec in a.precs.split(","):
        cfg, m, _ = make_model(28, precision=prec)
        for B in [int(b) for b in a.batches.split(",")]:
            fn = sampler(cfg, B, a.n)
            z = torch.randn(B, 63, device="cuda:0", generator=torch.Generator(device="cuda:0").manual_seed(B))
            for leg in legs:
                run(fn, m, z, leg)                                # warm-up
            ms = {leg: [] for leg in legs}
            outs = {}
            for _ in range(a.reps):
                for leg in legs:
                    t, outs[leg] = run(fn, m, z, leg)
                    ms[leg].append(t)
            r = {"prec": prec, "B": B}
            for leg in legs:
                r[f"{leg}_ms"] = float(np.median(ms[leg]))
                r[f"{leg}_all_ms"] = [float(v) for v in ms[leg]]
            if not a.only:
                d = (outs["fused"] - outs["generic"]).double()
                r["speedup"] = r["generic_ms"] / r["fused_ms"]
                r["max_abs_diff"] = float(d.abs().max())
                r["rel_l2_diff"] = float(d.norm() / outs["generic"].double().norm())
                r["bit_identical"] = bool(torch.equal(outs["fused"], outs["generic"]))
                r["finite"] = bool(torch.isfinite(outs["fused"]).all())
            res["runs"].append(r)
            print(json.dumps(r), flush=True)
            del fn, z, outs
            torch.cuda.empty_cache()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
