#!/usr/bin/env python3
"""Golden g28_pf_sampler: the reference's own pc_sampler with config.sampling.probability_flow = True (Euler-Maruyama predictor,
corrector 'none': deterministic sampling along the probability-flow ODE, sampling.py:182-188 with RSDE.sde of sde_lib.py:98-105), as
run/demo.py:437-450 decodes ODE latents with it -- captured by importing the reference (read-only); run in the build container only:

    python tests/golden/gen_golden_pf.py

* sub-VP, VP and VE at N = 8, B = 16 (eps = 1e-3);
* completion imputation (legs, sub-VP, N = 8): every torch.randn_like draw recorded in the reference's order, per step
  (impute-after-corrector, predictor z, impute-after-predictor) -- the predictor's z is multiplied by the zero diffusion;
* 'denoise' from start_step = 3 (sub-VP, N = 8);
* sub-VP at N = 1000, B = 8, eps = 1e-5 (demo.py:443): the final state and every 100th trajectory entry.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from gen_golden import Recorder, build_model, ref_misc, ref_sampling, ref_sde, save, toy_batch  # noqa: E402


def main():
    seed = 28
    cfg, m = build_model(seed, 63)
    m.eval()
    cfg.sampling.probability_flow = True
    cfg.sampling.predictor = "euler_maruyama"
    cfg.sampling.corrector = "none"
    out = {"seed": np.int64(seed), "sigma_min": np.float64(0.01), "sigma_max": np.float64(50.0)}
    kinds = {"subvp": lambda N: ref_sde.subVPSDE(0.1, 20.0, N), "vp": lambda N: ref_sde.VPSDE(0.1, 20.0, N),
             "ve": lambda N: ref_sde.VESDE(sigma_min=0.01, sigma_max=50.0, N=N)}

    class Args:
        task = None

    def run(tag, kind, N, B, eps, task=None, start_step=0, scale=1.0):
        sde = kinds[kind](N)
        fn = ref_sampling.get_sampling_fn(cfg, sde, (B, 63), lambda x: x, eps, device="cpu")
        z0 = torch.tensor((scale * np.random.RandomState(2800 + N + B + len(tag)).standard_normal((B, 63))).astype(np.float32))
        obs = mask = args = None
        if task is not None:
            args = Args()
            args.task = task
        if task == "completion":
            poses, _ = toy_batch(B, seed=44)
            with Recorder(55):
                mask, obs = ref_misc.create_mask(poses, part="legs")
            out[f"{tag}_mask"] = mask.numpy()
            out[f"{tag}_obs"] = obs.numpy()
        with Recorder(78) as rec:
            trajs, x = fn(m, observation=obs, mask=mask, z=z0, start_step=start_step, args=args)
        draws = rec.by_kind("randn")
        out[f"{tag}_z0"] = z0.numpy()
        out[f"{tag}_eps"] = np.float64(eps)
        out[f"{tag}_start_step"] = np.int64(start_step)
        if task == "completion":
            out[f"{tag}_noise"] = np.stack(draws)
        out[f"{tag}_n_draws"] = np.int64(len(draws))
        out[f"{tag}_final"] = x.numpy()
        tr = trajs.numpy()
        out[f"{tag}_trajs"] = tr if tr.shape[0] <= 16 else tr[99::100]

    for kind in ("subvp", "vp", "ve"):
        run(f"{kind}8", kind, 8, 16, 1e-3, scale=50.0 if kind == "ve" else 1.0)      # VE prior_sampling: N(0, sigma_max^2)
    run("comp8", "subvp", 8, 16, 1e-3, task="completion")
    run("den8", "subvp", 8, 16, 1e-3, task="denoise", start_step=3)
    run("pf1000", "subvp", 1000, 8, 1e-5)
    save("g28_pf_sampler", **out)


if __name__ == "__main__":
    main()
