"""Test infrastructure for the one-call MCG / DPS guided samplers (dposer_guided_sampler).

``guided_loop``: the loop of sampling.py:455-461 over EulerMaruyamaPredictor.update_fn_guide (sampling.py:191-207) on the CPU oracle --
``oracle.score_ref.em_guided_step`` (pinned to the reference by golden g16), for MCG followed by ``score_ref.impute`` (sampling.py:416-420,
pinned by g5).  No imputation ahead of the step, no corrector.  The dtype is that of the inputs.  ``noise`` has the library's slot layout
[n_run, 2 if mcg else 1, B, D]: the predictor's z, then the imputation draw.  ``forced`` [n_run, B, D] teacher-forces the loop: index i
steps from ``forced[i]`` instead of from its own previous state.

Golden g33 (tests/golden/gen_golden_guided.py): ``golden_cases`` / ``case_inputs`` rebuild a case's inputs from the stored seeds.
"""
import numpy as np
import torch

from oracle import score_ref as R

METHODS = ("dps", "mcg")


def noise_slots(method):
    return 2 if method == "mcg" else 1


def oracle_sde(kind, N):
    return (R.SubVP if kind == "subvp" else R.VP)(0.1, 20.0, N)


def params_as(p, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in p.items()}


def guided_loop(p, sde, x_init, noise, observation, mask, *, method, grad_step=1.0, eps=1e-3, start_step=0, run_steps=-1, forced=None, **fw):
    """Returns (trajs [n, B, D], x, x_mean)."""
    assert method in METHODS
    dt = x_init.dtype
    p = params_as(p, dt)
    obs, msk = torch.as_tensor(observation).to(dt), torch.as_tensor(mask).to(dt)
    timesteps = torch.linspace(sde.T, eps, sde.N).to(dt)                     # sampling.py:449
    n_run = sde.N - start_step if run_steps < 0 else run_steps
    x = x_mean = x_init
    trajs = []
    for k in range(n_run):
        i = start_step + k
        if forced is not None:
            x = torch.as_tensor(forced[k]).to(dt)
        vec_t = torch.ones(x.shape[0], dtype=dt) * timesteps[i]              # :458
        z = torch.as_tensor(noise[k, 0]).to(dt)
        x, x_mean = R.em_guided_step(p, sde, x, vec_t, z, obs, msk, grad_step=grad_step, **fw)
        x, x_mean = x.detach(), x_mean.detach()
        if method == "mcg":
            x = R.impute(sde, x, vec_t, obs, msk, torch.as_tensor(noise[k, 1]).to(dt))
        trajs.append(x)
    return torch.stack(trajs, 0), x, x_mean


# ---- golden g33: tags and inputs ---------------------------------------------------------------------------------------------------------
def golden_cases():
    from helpers import load
    return [str(t) for t in load("g33_guided_sampler")["cases"]]


def case_inputs(g, tag):
    """'<kind>_<method>_N<N>_s<start>': the inputs of a case, its draws regenerated from the stored seeds in the reference's order."""
    kind, method = tag.split("_")[:2]
    N, B, start, z0_seed, n_draws, keep = (int(v) for v in g[f"{tag}_meta"])
    n_run, slots = N - start, noise_slots(method)
    assert n_draws == n_run * slots
    rs = np.random.RandomState(int(g["noise_seed"]))
    noise = np.stack([rs.standard_normal((B, 63)).astype(np.float32) for _ in range(n_draws)]).reshape(n_run, slots, B, 63)
    return dict(kind=kind, method=method, N=N, B=B, start=start, keep=keep, noise=noise, x0=g[f"{tag}_x0"], obs=g["obs"], mask=g["mask"],
                grad_step=float(g["grad_step"]), eps=float(g["eps"]))
