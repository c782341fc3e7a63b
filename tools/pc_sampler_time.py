#!/usr/bin/env python3
"""Times pc_sampler's one-call path (dposer_pc_sampler) against what ran before it, on one GPU: 500 poses x N = 1000, eps = 5e-3,
sub-VP, ScoreModelFC (H = 1024, 2 blocks, D = 63), no trajectory kept.

  em+langevin        one call  vs  fused_pc_langevin_sample (three library calls and a host table read per step: the path before)
  reverse_diffusion  one call  vs  the generic torch loop over the HIP score function
  em+ald             one call  vs  the generic torch loop

Device events around each call, one warm-up call per leg, `--repeats` repeats alternating between the legs; median and min-max in ms.
The "before" legs run in the same process on the same GPU: fused_pc_langevin_sample is the unchanged per-step path, and the generic
loop is reached by making fused_pc_supported answer False for the call.  Prints a markdown table (profiles/pc_sampler_time.md).
`--big` is the run for a kernel trace of k_pc_pred_update / k_ald_update at a large batch."""
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
    ap.add_argument("--batch", type=int, default=500)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--big", action="store_true", help="one reverse_diffusion + ald call at --batch x --steps after a warm-up call, nothing "
                    "else: the run to put under a kernel trace for the two update kernels' time per launch")
    a = ap.parse_args()
    from gpu_common import make_model
    from dposer_amd.algorithms.advanced import sampling, sde_lib
    dev = "cuda:0"
    cfg, m, _ = make_model(3, precision=a.precision)
    sde = sde_lib.subVPSDE(0.1, 20.0, a.steps)
    z = torch.randn(a.batch, 63, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    ts = torch.linspace(sde.T, 5e-3, sde.N)
    EM, RD = sampling.EulerMaruyamaPredictor, sampling.ReverseDiffusionPredictor
    NONE, LANG, ALD = sampling.NoneCorrector, sampling.LangevinCorrector, sampling.AnnealedLangevinDynamics

    def one_call(pred, corr):
        return lambda: sampling.fused_pc_sample(m, sde, z, ts, predictor=pred, corrector=corr, snr=0.16, n_steps=1, seed=2)[1]

    def generic(pred, corr):
        fn = sampling.get_pc_sampler(sde, (a.batch, 63), pred, corr, lambda v: v, 0.16, n_steps=1, continuous=True, eps=5e-3, device=dev)

        def run():
            keep = sampling.fused_pc_supported
            sampling.fused_pc_supported = lambda *x, **k: False
            try:
                return fn(m, z=z, traj_stride=0)[1]
            finally:
                sampling.fused_pc_supported = keep
        return run

    if a.big:
        run = one_call(RD, ALD)
        for _ in range(2):
            assert torch.isfinite(run()).all()
        torch.cuda.synchronize()
        print(f"big: reverse_diffusion + ald, B = {a.batch}, N = {a.steps}, {a.precision}: two calls done")
        return

    legs = [("euler_maruyama + langevin", one_call(EM, LANG), "three calls per step",
             lambda: sampling.fused_pc_langevin_sample(m, sde, z, ts, snr=0.16, n_steps=1, seed=2)[1]),
            ("reverse_diffusion + none", one_call(RD, NONE), "generic loop", generic(RD, NONE)),
            ("euler_maruyama + ald", one_call(EM, ALD), "generic loop", generic(EM, ALD))]

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        out = f()
        e1.record()
        torch.cuda.synchronize()
        assert torch.isfinite(out).all()
        return e0.elapsed_time(e1)

    print(f"| pair | B | N | one call: median (min-max) ms | before: path | before: median (min-max) ms | speed-up |")
    print("|---|---:|---:|---:|---|---:|---:|")
    for name, new, old_name, old in legs:
        timed(new), timed(old)
        tn, to = [], []
        for _ in range(a.repeats):
            tn.append(timed(new))
            to.append(timed(old))
        mn, mo = statistics.median(tn), statistics.median(to)
        print(f"| {name} | {a.batch} | {a.steps} | {mn:.1f} ({min(tn):.1f}-{max(tn):.1f}) | {old_name} | {mo:.1f} ({min(to):.1f}-{max(to):.1f}) | {mo / mn:.2f}x |",
              flush=True)


if __name__ == "__main__":
    main()
