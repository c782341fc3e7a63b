"""Test infrastructure: the probability-flow pc_sampler (sampling.py:182-188 with RSDE.sde of sde_lib.py:98-105, corrector 'none',
imputation :416-420) built on the CPU oracle: the drift of ``oracle.score_ref.rsde_sde(..., probability_flow=True)``, x = x_mean (the
reference's diffusion is zeros(1)), and ``oracle.score_ref.impute`` around the predictor when a completion is asked for."""
import torch

from oracle import score_ref as R


def pf_sampler(p, sde, x_init, *, eps=1e-3, start_step=0, observation=None, mask=None, impute_noises=None, keep_traj=True, **fw):
    """Loop indices [start_step, sde.N).  ``impute_noises[i]`` = (impute-after-corrector, impute-after-predictor) draws of loop index i.
    Returns (trajs [n, B, D] or None, x_mean of the last step)."""
    x = x_init
    timesteps = torch.linspace(sde.T, eps, sde.N).to(x.dtype)                # sampling.py:449
    dt = -1.0 / sde.N
    trajs = []
    x_mean = x
    for i in range(start_step, sde.N):
        vec_t = torch.ones(x.shape[0], dtype=x.dtype) * timesteps[i]         # :458
        if observation is not None:
            x = R.impute(sde, x, vec_t, observation, mask, impute_noises[i][0])
        drift, _, _ = R.rsde_sde(p, sde, x, vec_t, probability_flow=True, **fw)
        x_mean = x + drift * dt                                              # :186
        x = x_mean                                                           # :187 with diffusion zeros(1)
        if observation is not None:
            x = R.impute(sde, x, vec_t, observation, mask, impute_noises[i][1])
        if keep_traj:
            trajs.append(x)
    return (torch.stack(trajs, 0) if keep_traj else None), x_mean
