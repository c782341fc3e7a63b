#!/usr/bin/env python3
"""Times the one-call MCG / DPS guided sampler (dposer_guided_sampler) against the per-step loop that ran before it, on one GPU: N = 1000,
eps = 1e-3, sub-VP, ScoreModelFC (H = 1024, 2 blocks, D = 63), legs masked, no trajectory kept, B = 500 (config 3's size) and B = 16384
(the completion batch), fp32 and bf16.

  one call   sampling.get_guided_sampler on the supported pair: one library call and one 4-byte read per run
  per step   the same factory with the one-call path switched off: EulerMaruyamaPredictor.update_fn_guide (an autograd round trip
             through the HIP forward / input-gradient pair and an isnan(...).any() read per step) + the imputation expression in torch --
             what a user's loop over the shipped step ran before

Device events around each run, one warm-up run per leg, `--repeats` repeats alternating between the legs; median and min-max in ms.
Both legs run in the same process on the same GPU.  Their draws differ (Philox in the kernel, torch's generator in the loop), so each
result is only checked to be finite here; tests/test_gpu_guided_sampler.py compares the two paths' numbers with injected draws.
Launches: the library's GEMM launches per step of each leg are counted by the library's own launch records in a short run of its own
(`--count-steps`); the one-call path adds 3 elementwise launches per step (k_guided_resid, k_sum_partials, k_guided_update), the
per-step loop torch's own kernels (not counted here).  Prints a markdown table (profiles/guided_sampler_time.md)."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[500, 16384])
    ap.add_argument("--precisions", nargs="+", default=["fp32", "bf16"])
    ap.add_argument("--methods", nargs="+", default=["mcg", "dps"])
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--count-steps", type=int, default=8)
    a = ap.parse_args()
    from gpu_common import make_model
    from dposer_amd import _C
    from dposer_amd.algorithms.advanced import sampling, sde_lib
    from dposer_amd.utils.misc import create_mask
    assert torch.cuda.is_available(), "guided_time.py measures on the GPU"
    dev = "cuda:0"

    def legs(m, sde, B, method):
        g = torch.Generator(device=dev).manual_seed(1)
        z = torch.randn(B, 63, device=dev, generator=g)
        mask, obs = create_mask(0.5 * torch.randn(B, 63, device=dev, generator=g), part="legs")
        fn = sampling.get_guided_sampler(sde, (B, 63), lambda v: v, method, grad_step=0.5, eps=1e-3, device=dev)

        def new():
            return fn(m, obs, mask, z=z, traj_stride=0, seed=2)[1]

        def old():
            keep = sampling.fused_guided_supported
            sampling.fused_guided_supported = lambda *x, **k: False
            try:
                return fn(m, obs, mask, z=z, traj_stride=0)[1]
            finally:
                sampling.fused_guided_supported = keep
        return new, old

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        out = f()
        e1.record()
        torch.cuda.synchronize()
        assert torch.isfinite(out).all()
        return e0.elapsed_time(e1)

    def gemm_launches(f):
        _C.profile_enable(True)
        f()
        torch.cuda.synchronize()
        n = sum(v[1] for v in _C.profile_collect().values())
        _C.profile_enable(False)
        return n

    print("| method | precision | B | N | one call: median (min-max) ms | per step: median (min-max) ms | speed-up | GEMM launches per step: one call / per step |")
    print("|---|---|---:|---:|---:|---:|---:|---:|")
    for prec in a.precisions:
        cfg, m, _ = make_model(3, precision=prec)
        for B in a.batches:
            for method in a.methods:
                new, old = legs(m, sde_lib.subVPSDE(0.1, 20.0, a.steps), B, method)
                timed(new), timed(old)
                tn, to = [], []
                for _ in range(a.repeats):
                    tn.append(timed(new))
                    to.append(timed(old))
                cn, co = legs(m, sde_lib.subVPSDE(0.1, 20.0, a.count_steps), B, method)
                cn(), co()
                ln, lo = gemm_launches(cn) / a.count_steps, gemm_launches(co) / a.count_steps
                mn, mo = statistics.median(tn), statistics.median(to)
                print(f"| {method} | {prec} | {B} | {a.steps} | {mn:.1f} ({min(tn):.1f}-{max(tn):.1f}) | {mo:.1f} ({min(to):.1f}-{max(to):.1f}) | "
                      f"{mo / mn:.2f}x | {ln:.2f} / {lo:.2f} |", flush=True)


if __name__ == "__main__":
    main()
