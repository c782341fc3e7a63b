#!/usr/bin/env python3
"""Multi-step (DDIM) prior loss and RED-Diff: the one call (dposer_prior_loss_multi / dposer_prior_red_diff through prior_loss(...,
multi_denoise=N) / red_diff) against the unfused composition of dposer_amd/prior.py (N calls of the HIP score function + torch elementwise
operations: what a user had to write before the entries existed), alternating on the same device from the same poses and the same injected z.
Each timed call is the loss AND its gradient w.r.t. the poses (loss.backward()).

    python tools/prior_variants_time.py [--batches 128,16384] [--precs bf16,bf16x3] [--iters 20] [--reps 5] [--out prior_variants_time.json]
    python tools/prior_variants_time.py --only fused|unfused --batches 128 --precs bf16 --reps 1      (one leg alone, for kernel traces)

Device events around --iters back-to-back calls, one warm-up round per leg; the median over --reps alternating rounds, per call.  The losses
and gradients of the two legs of the last round are compared.  Writes one JSON and prints the table rows."""
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

VARIANTS = {"multi5": 5, "multi10": 10, "red_diff": 0}
T = 0.3


def call(m, sde, x0, z, variant, leg):
    """One evaluation of loss and gradient; returns (loss, d loss / d x0)."""
    from dposer_amd import prior
    x = x0.clone().requires_grad_(True)
    n = VARIANTS[variant]
    if leg == "fused":
        loss = prior.prior_loss(m, sde, x, T, weighted=True, z=z, multi_denoise=n) if n else prior.red_diff(m, sde, x, T, z=z)
    elif n:
        loss = prior._prior_loss_multi_unfused(m, sde, x, prior.multi_step_time_grid(T, n), True, 1.0 / x.numel(), z)
    else:
        loss = prior._red_diff_unfused(m, sde, x, T, z)
    loss.backward()
    return loss.detach(), x.grad


def timed(m, sde, x0, z, variant, leg, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        out = call(m, sde, x0, z, variant, leg)
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / iters, out


def main():
    from dposer_amd.algorithms.advanced import sde_lib
    from gpu_common import make_model
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="128,16384")
    ap.add_argument("--precs", default="bf16,bf16x3")
    ap.add_argument("--variants", default="multi5,multi10,red_diff")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=["fused", "unfused"], default=None)
    ap.add_argument("--out", default="prior_variants_time.json")
    a = ap.parse_args()
    legs = [a.only] if a.only else ["fused", "unfused"]
    sde = sde_lib.subVPSDE(0.1, 20.0, 1000)
    res = {"t": T, "sde": "subVPSDE(0.1, 20, 1000)", "network": "ScoreModelFC H = 1024, 2 blocks, D = 63", "iters": a.iters, "reps": a.reps,
           "timed": "loss + gradient w.r.t. the poses, per call", "runs": []}
    rows = []
    for prec in a.precs.split(","):
        cfg, m, _ = make_model(31, precision=prec)
        m.freeze_packed = True                                    # the weights do not change between calls: packed once, as the task loops do
        for B in [int(b) for b in a.batches.split(",")]:
            gen = torch.Generator(device="cuda:0").manual_seed(B)
            x0 = torch.randn(B, 63, device="cuda:0", generator=gen)
            z = torch.randn(B, 63, device="cuda:0", generator=gen)
            for variant in a.variants.split(","):
                for leg in legs:
                    timed(m, sde, x0, z, variant, leg, 2)         # warm-up
                ms = {leg: [] for leg in legs}
                outs = {}
                for _ in range(a.reps):
                    for leg in legs:
                        t, outs[leg] = timed(m, sde, x0, z, variant, leg, a.iters)
                        ms[leg].append(t)
                r = {"prec": prec, "B": B, "variant": variant}
                for leg in legs:
                    r[f"{leg}_ms"] = float(np.median(ms[leg]))
                    r[f"{leg}_all_ms"] = [float(v) for v in ms[leg]]
                if not a.only:
                    (lf, gf), (lu, gu) = outs["fused"], outs["unfused"]
                    r["speedup"] = r["unfused_ms"] / r["fused_ms"]
                    r["loss_rel_diff"] = float((lf - lu).abs() / lu.abs())
                    r["grad_rel_l2_diff"] = float((gf - gu).double().norm() / gu.double().norm())
                    r["finite"] = bool(torch.isfinite(gf).all() and torch.isfinite(lf))
                    rows.append(f"| {prec} | {B} | {variant} | {r['fused_ms']:.3f} | {r['unfused_ms']:.3f} | {r['speedup']:.2f}× | "
                                f"{r['loss_rel_diff']:.1e} | {r['grad_rel_l2_diff']:.1e} |")
                res["runs"].append(r)
                print(json.dumps(r), flush=True)
            del x0, z
            torch.cuda.empty_cache()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    if rows:
        print("| precision | B | variant | one call (ms) | unfused (ms) | speed-up | loss rel diff | grad rel L2 diff |")
        print("|---|---:|---|---:|---:|---:|---:|---:|")
        print("\n".join(rows))


if __name__ == "__main__":
    main()
