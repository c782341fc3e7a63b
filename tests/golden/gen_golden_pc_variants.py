#!/usr/bin/env python3
"""Golden g32_pc_variants: the reference's predictors and correctors other than Euler-Maruyama + 'none' -- ReverseDiffusionPredictor,
AncestralSamplingPredictor, NonePredictor, LangevinCorrector, AnnealedLangevinDynamics (sampling.py:210-339) -- stepped in the order of
pc_sampler (sampling.py:455-461), captured by importing the reference (read-only); run in the build container only:

    python tests/golden/gen_golden_pc_variants.py

The reference's own pc_sampler cannot run 'reverse_diffusion' or 'ancestral_sampling' (their update_fn(x, t) is called with four
arguments, and the ancestral predictor calls score_fn(x, t) without condition / mask), so those combinations are stepped by the loop
below on the reference's own Predictor / Corrector objects -- keys tagged ``loop`` -- with the ancestral predictor's score function
wrapped to two arguments.  Where get_sampling_fn can run the combination (Euler-Maruyama or 'none' predictor with 'ald') it does -- keys
tagged ``fn``.

N = 32, B = 8, D = 63, eps = 1e-3, sub-VP / VP / VE (VE's prior scaled by sigma_max = 50); beta_max = 20 makes alphas = 1 - discrete_betas
negative below N = 21, hence not N = 8.  Every 4th trajectory entry is kept; the N = 1000 cases keep every 100th.  The draws are NOT
stored: the Recorder's seed and the number of draws are, and this script asserts that RandomState(seed).standard_normal((B, 63)) in
sequence reproduces what was recorded.  z0 is RandomState(z0_seed).standard_normal((B, 63)) * z0_scale as float32.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from gen_golden import Recorder, build_model, ref_misc, ref_mutils, ref_sampling, ref_sde, save, toy_batch  # noqa: E402

SEED, NOISE_SEED, SNR = 32, 79, 0.16
KINDS = {"subvp": lambda N: ref_sde.subVPSDE(0.1, 20.0, N), "vp": lambda N: ref_sde.VPSDE(0.1, 20.0, N),
         "ve": lambda N: ref_sde.VESDE(sigma_min=0.01, sigma_max=50.0, N=N)}
SHORT = {"reverse_diffusion": "rd", "ancestral_sampling": "anc", "euler_maruyama": "em", "none": "none", "langevin": "lang", "ald": "ald"}


class Args:
    task = None


def stepped(sde, m, predictor, corrector, n_each, pf, x, eps, start_step, obs, mask):
    """sampling.py:455-461 on the reference's own objects."""
    score_fn = ref_mutils.get_score_fn(sde, m, train=False, continuous=True)
    two = lambda a, t: score_fn(a, t, None, None)
    pred = ref_sampling.get_predictor(predictor)(sde, two if predictor == "ancestral_sampling" else score_fn, pf)
    corr = ref_sampling.get_corrector(corrector)(sde, score_fn, SNR, n_each)
    timesteps = torch.linspace(sde.T, eps, sde.N)
    trajs = []
    x_mean = x

    def impute(x, vec_t):                                                    # :416-420
        mean, std = sde.marginal_prob(obs, vec_t)
        return x * (1 - mask) + (mean + torch.randn_like(x) * std[:, None]) * mask

    with torch.no_grad():
        for i in range(start_step, sde.N):
            vec_t = torch.ones(x.shape[0]) * timesteps[i]
            x, x_mean = corr.update_fn(x, vec_t, obs, mask)
            if obs is not None:
                x = impute(x, vec_t)
            x, x_mean = pred.update_fn(x, vec_t) if predictor in ("reverse_diffusion", "ancestral_sampling") else pred.update_fn(x, vec_t, obs, mask)
            if obs is not None:
                x = impute(x, vec_t)
            trajs.append(x)
    return torch.stack(trajs, 0), x_mean


def main():
    cfg, m = build_model(SEED, 63)
    m.eval()
    out = {"seed": np.int64(SEED), "noise_seed": np.int64(NOISE_SEED), "snr": np.float64(SNR), "sigma_min": np.float64(0.01),
           "sigma_max": np.float64(50.0), "cases": []}
    for N in (32, 1000):
        out[f"ve_discrete_sigmas_{N}"] = KINDS["ve"](N).discrete_sigmas.numpy()
        out[f"vp_discrete_betas_{N}"] = KINDS["vp"](N).discrete_betas.numpy()

    def run(kind, predictor, corrector, *, n_each=1, pf=False, N=32, B=8, eps=1e-3, task=None, start_step=0, keep=4, use_fn=False, traj=True):
        tag = f"{kind}_{SHORT[predictor]}_{SHORT[corrector]}" + (f"{n_each}" if n_each != 1 else "") + ("_pf" if pf else "") + \
              (f"_{task}" if task else "") + (f"_N{N}" if N != 32 else "") + ("_fn" if use_fn else "_loop")
        sde = KINDS[kind](N)
        z0_seed = 3200 + len(out["cases"])
        scale = 50.0 if kind == "ve" else 1.0
        z0 = torch.tensor((scale * np.random.RandomState(z0_seed).standard_normal((B, 63))).astype(np.float32))
        obs = mask = None
        if task == "completion":
            poses, _ = toy_batch(B, seed=44)
            with Recorder(55):
                mask, obs = ref_misc.create_mask(poses, part="legs")
            out[f"{tag}_mask"] = mask.numpy()
            out[f"{tag}_obs"] = obs.numpy()
        with Recorder(NOISE_SEED) as rec:
            if use_fn:
                cfg.sampling.predictor, cfg.sampling.corrector = predictor, corrector
                cfg.sampling.n_steps_each, cfg.sampling.snr, cfg.sampling.probability_flow = n_each, SNR, pf
                args = None
                if task is not None:
                    args = Args()
                    args.task = task
                trajs, x = ref_sampling.get_sampling_fn(cfg, sde, (B, 63), lambda v: v, eps, device="cpu")(
                    m, observation=obs, mask=mask, z=z0, start_step=start_step, args=args)
            else:
                trajs, x = stepped(sde, m, predictor, corrector, n_each, pf, z0, eps, start_step if task == "denoise" else 0, obs, mask)
        draws = rec.by_kind("randn")
        rs = np.random.RandomState(NOISE_SEED)
        for d in draws:                                                      # the tests regenerate the draws exactly like this
            assert np.array_equal(d, rs.standard_normal((B, 63)).astype(np.float32))
        assert torch.isfinite(trajs).all() and torch.isfinite(x).all(), tag
        out["cases"].append(tag)
        out[f"{tag}_meta"] = np.asarray([N, B, n_each, int(pf), start_step if task == "denoise" else 0, z0_seed, len(draws), keep], np.int64)
        out[f"{tag}_eps"] = np.float64(eps)
        out[f"{tag}_z0_scale"] = np.float64(scale)
        out[f"{tag}_final"] = x.numpy()
        if traj:
            out[f"{tag}_trajs"] = trajs.numpy()[keep - 1::keep]

    for kind in ("subvp", "vp", "ve"):
        run(kind, "reverse_diffusion", "none")
    for kind in ("vp", "ve"):
        run(kind, "ancestral_sampling", "none")
    run("subvp", "none", "none", use_fn=True, traj=False)                    # (the identity: every trajectory entry is z0)
    for kind in ("subvp", "vp", "ve"):
        run(kind, "reverse_diffusion", "none", pf=True)
    run("subvp", "euler_maruyama", "ald", use_fn=True)
    run("ve", "none", "ald", use_fn=True)
    run("vp", "reverse_diffusion", "ald")
    run("ve", "reverse_diffusion", "ald")
    run("subvp", "reverse_diffusion", "ald", n_each=2)
    for kind in ("vp", "ve"):
        run(kind, "ancestral_sampling", "ald")
    for kind in ("subvp", "vp", "ve"):
        run(kind, "reverse_diffusion", "langevin")
    run("subvp", "reverse_diffusion", "ald", task="completion")
    run("vp", "reverse_diffusion", "ald", task="denoise", start_step=5)
    for kind in ("subvp", "ve"):
        run(kind, "reverse_diffusion", "ald", N=1000, keep=100)
    out["cases"] = np.asarray(out["cases"])
    save("g32_pc_variants", **out)


if __name__ == "__main__":
    main()
