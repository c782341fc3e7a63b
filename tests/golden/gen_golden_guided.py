#!/usr/bin/env python3
"""Golden g33_guided_sampler: the MCG and DPS completion loops -- the reference's own EulerMaruyamaPredictor.update_fn_guide
(sampling.py:191-207) stepped in the order of pc_sampler (sampling.py:455-461), for MCG followed by the imputation expression of
:416-420 -- captured by importing the reference (read-only); run in the build container only:

    python tests/golden/gen_golden_guided.py

(sub-VP, VP) x (dps, mcg), D = 63, B = 8, legs masked via create_mask, grad_step = 0.7, eps = 1e-3:
    N = 1000 from index 600 (x starts as the observation perturbed to t[600]), N = 1000 from 0, N = 32 from 0 (x starts as the prior draw).
Every 100th (N = 1000) or 4th (N = 32) state is kept, plus the final x and x_mean.  The draws are NOT stored: the Recorder's seed and the
number of draws are, and this script asserts that RandomState(seed).standard_normal((B, 63)) in sequence reproduces what was recorded
(per index: the predictor's z, then MCG's imputation draw).  The start states are stored (2 KiB each).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from gen_golden import Recorder, build_model, ref_misc, ref_mutils, ref_sampling, ref_sde, save, toy_batch  # noqa: E402

SEED, NOISE_SEED, GRAD_STEP, EPS, B = 33, 83, 0.7, 1e-3, 8
KINDS = {"subvp": lambda N: ref_sde.subVPSDE(0.1, 20.0, N), "vp": lambda N: ref_sde.VPSDE(0.1, 20.0, N)}


def stepped(sde, m, method, x, start_step, obs, mask, keep):
    score_fn = ref_mutils.get_score_fn(sde, m, train=False, continuous=True)
    pred = ref_sampling.EulerMaruyamaPredictor(sde, score_fn, probability_flow=False)
    timesteps = torch.linspace(sde.T, EPS, sde.N)
    kept = []
    x_mean = x
    for i in range(start_step, sde.N):
        vec_t = torch.ones(x.shape[0]) * timesteps[i]
        x, x_mean = pred.update_fn_guide(x.detach(), vec_t, obs, mask, grad_step=GRAD_STEP)
        x, x_mean = x.detach(), x_mean.detach()
        if method == "mcg":                                                  # sampling.py:416-420
            mean, std = sde.marginal_prob(obs, vec_t)
            x = x * (1 - mask) + (mean + torch.randn_like(x) * std[:, None]) * mask
        if (i - start_step + 1) % keep == 0:
            kept.append(x)
    return torch.stack(kept, 0), x, x_mean


def main():
    cfg, m = build_model(SEED, 63)
    m.eval()
    poses, _ = toy_batch(B, seed=47)
    with Recorder(57):
        mask, obs = ref_misc.create_mask(poses, part="legs")
    out = {"seed": np.int64(SEED), "noise_seed": np.int64(NOISE_SEED), "grad_step": np.float64(GRAD_STEP), "eps": np.float64(EPS),
           "mask": mask.numpy(), "obs": obs.numpy(), "cases": []}
    for kind in ("subvp", "vp"):
        for method in ("dps", "mcg"):
            for N, start, keep in ((1000, 600, 100), (1000, 0, 100), (32, 0, 4)):
                tag = f"{kind}_{method}_N{N}_s{start}"
                sde = KINDS[kind](N)
                z0_seed = 3300 + len(out["cases"])
                z0 = torch.tensor(np.random.RandomState(z0_seed).standard_normal((B, 63)).astype(np.float32))
                if start:
                    vec_t = torch.ones(B) * torch.linspace(sde.T, EPS, sde.N)[start]
                    mean, std = sde.marginal_prob(obs, vec_t)
                    x0 = mean + std[:, None] * z0
                else:
                    x0 = z0
                with Recorder(NOISE_SEED) as rec:
                    kept, x, x_mean = stepped(sde, m, method, x0, start, obs, mask, keep)
                draws = rec.by_kind("randn")
                rs = np.random.RandomState(NOISE_SEED)
                for d in draws:                                              # the tests regenerate the draws exactly like this
                    assert np.array_equal(d, rs.standard_normal((B, 63)).astype(np.float32))
                assert len(draws) == (N - start) * (2 if method == "mcg" else 1)
                assert torch.isfinite(kept).all() and torch.isfinite(x).all() and torch.isfinite(x_mean).all(), tag
                print(tag, "max |x| kept", float(kept.abs().max()))
                out["cases"].append(tag)
                out[f"{tag}_meta"] = np.asarray([N, B, start, z0_seed, len(draws), keep], np.int64)
                out[f"{tag}_x0"] = x0.numpy()
                out[f"{tag}_trajs"] = kept.numpy()
                out[f"{tag}_final"] = x.numpy()
                out[f"{tag}_final_mean"] = x_mean.numpy()
    out["cases"] = np.asarray(out["cases"])
    save("g33_guided_sampler", **out)


if __name__ == "__main__":
    main()
