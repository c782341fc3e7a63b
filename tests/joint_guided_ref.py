"""The float64 rule of the joints-only kinematic chain: what ``dposer_fk_joints`` computes and, by autograd, what
``dposer_fk_joints_backward`` returns.  TEST INFRASTRUCTURE: rotations are ``oracle.fk_torch.batch_rodrigues`` (smplx's, with its
``+ 1e-8``), the chain is smplx ``batch_rigid_transform`` restricted to the joint positions -- no vertex is formed, so a reference
over 55 joints of a few hundred poses costs milliseconds."""
import torch

from oracle import fk_torch

SMPLX_PARENTS = (-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 15, 15, 15, 20, 25, 26, 20, 28, 29, 20, 31, 32,
                 20, 34, 35, 20, 37, 38, 21, 40, 41, 21, 43, 44, 21, 46, 47, 21, 49, 50, 21, 52, 53)


def fk_chain(full_pose, j_rest, parents, n_out, transl=None):
    """Posed joints [B, n_out, 3] of ``full_pose [B, J * 3]`` (axis-angle, root first) over rest joints ``j_rest [J, 3]`` or
    ``[B, J, 3]``; every tensor in the dtype of ``full_pose``."""
    B = full_pose.shape[0]
    J = len(parents)
    R = fk_torch.batch_rodrigues(full_pose.reshape(-1, 3)).view(B, J, 3, 3)
    jr = j_rest if j_rest.dim() == 3 else j_rest[None].expand(B, J, 3)
    RG, t = [R[:, 0]], [jr[:, 0]]
    for i in range(1, n_out):
        p = parents[i]
        RG.append(RG[p] @ R[:, i])
        t.append((RG[p] @ (jr[:, i] - jr[:, p])[..., None])[..., 0] + t[p])
    posed = torch.stack(t, dim=1)
    return posed if transl is None else posed + transl[:, None]


def fk22(pose, root, j_rest, transl=None):
    """The 22 body joints of an SMPL-X body: ``pose [B, 63]``, ``root [B, 3]`` or None (identity), hands and face at rest."""
    B = pose.shape[0]
    z = lambda n: torch.zeros(B, n, dtype=pose.dtype)
    full = torch.cat([root if root is not None else z(3), pose, z(3 * (len(SMPLX_PARENTS) - 22))], dim=1)
    return fk_chain(full, j_rest, SMPLX_PARENTS, 22, transl)


def denormalise(y0, mode, a, b):
    """offline_denormalize of dposer_amd/dataset/AMASS.py: mode 0 identity, 1 z-score (a = mean, b = std), 2 min-max (a = min, b = max)."""
    if mode == 1:
        return y0 * b + a
    if mode == 2:
        return 0.5 * ((y0 + 1) * (b - a) + 2 * a)
    return y0


def live_entries(obs, conf):
    """(live [B, n_obs] bool, c [B, n_obs] with zeros where dead, obs with zeros where dead): an entry is live iff c > 0 -- false for 0,
    for negatives and for NaN; what lies under a dead entry never enters a sum."""
    B, n_obs = obs.shape[:2]
    c = torch.ones(B, n_obs, dtype=obs.dtype) if conf is None else conf.to(obs.dtype)
    live = c > 0
    return live, torch.where(live, c, torch.zeros_like(c)), torch.where(live[..., None], obs, torch.zeros_like(obs))


def stage_sum(y0, mode, a, b, root, transl, j_rest, obs, conf, rows):
    """s[b] = sum_live c |J_rows[j](denormalise(y0)) - o_j|^2, differentiable in y0; every tensor in y0's dtype."""
    J = fk22(denormalise(y0, mode, a, b), root, j_rest, transl)
    idx = list(range(obs.shape[1])) if rows is None else [int(r) for r in rows]
    _, c, o = live_entries(obs, conf)
    r = J[:, idx] - o
    return (c * (r * r).sum(dim=2)).sum(dim=1)


def joint_stage(y0, mode, a, b, root, transl, j_rest, obs, conf=None, rows=None):
    """(s [B], v [B, 63] = 1/2 ds/dy0) by autograd, in the dtype of ``y0`` (float64: the rule; float32: its own rounding)."""
    y = y0.detach().clone().requires_grad_(True)
    s = stage_sum(y, mode, a, b, root, transl, j_rest, obs, conf, rows)
    (g,) = torch.autograd.grad(s.sum(), [y])
    return s.detach(), 0.5 * g


def joint_guided_step(p, sde, x_t, t, z, stage, *, norm, grad_step, group=None, **fw):
    """One index of DPS on observed 3D joints -- oracle.score_ref.em_guided_step with the stage's norm for the masked one:
    y0 = (x + sigma^2 score) / alpha;  s = stage_sum(y0);  norm = sqrt(sum_b s[b]) ("batch") or sqrt(s[b]) ("sample");
    x' = y_hat - grad_step d norm / d x, the gradient taken as 0 where the norm is 0.  ``stage``: the keyword arguments of
    ``stage_sum`` behind y0, already in the dtype of ``x_t``.  ``group``: the rows are consecutive batches of ``group`` rows (each with its
    own t), stepped side by side -- "batch" norms are then taken per batch.  Returns (x', y_mean, s)."""
    import numpy as np
    from oracle import score_ref as R
    x = x_t.detach().clone().requires_grad_(True)
    dt = -1.0 / sde.N
    drift, g, score = R.rsde_sde(p, sde, x, t, **fw)
    alpha, sigma = sde.alpha_sigma(t)
    y_mean = x.detach() + drift.detach() * dt
    y_hat = y_mean + g[:, None] * np.sqrt(-dt) * z
    y0 = (x + (sigma ** 2)[:, None] * score) / alpha
    s = stage_sum(y0, **stage)
    sn = s.reshape(-1, group or s.shape[0]).sum(dim=1) if norm == "batch" else s
    on = sn > 0
    total = torch.where(on, torch.sqrt(torch.where(on, sn, torch.ones_like(sn))), torch.zeros_like(sn)).sum()
    grad = torch.autograd.grad(total, x)[0] if bool(on.any()) else torch.zeros_like(y_hat)
    bad = ~torch.isfinite(sn)
    if bool(bad.any()):                              # a NaN / Inf observation under a positive confidence: its norm's rows are not finite
        rows_bad = bad.repeat_interleave(group or s.shape[0]) if norm == "batch" else bad
        grad = torch.where(rows_bad[:, None], torch.full_like(grad, float("nan")), grad)
    return (y_hat - grad_step * grad).detach(), y_mean, s.detach()


def joint_guided_loop(p, sde, x_init, noise, joints_obs, conf, rows, *, mode=0, a=None, b=None, root=None, transl=None, j_rest=None, norm="sample",
                      grad_step=1.0, eps=1e-3, start_step=0, run_steps=-1, forced=None, dtype=None, **fw):
    """The loop of sampling.py:455-461 over ``joint_guided_step``.  ``noise`` [n_run, 1, B, D]; ``forced`` [n_run, B, D] teacher-forces it:
    index i steps from ``forced[i]``.  Everything runs in ``dtype`` (default: that of ``x_init``).  Returns (trajs [n, B, D], x, x_mean)."""
    from guided_ref import params_as
    dt = dtype or x_init.dtype
    cast = lambda v: None if v is None else torch.as_tensor(v).to(dt)
    p = params_as(p, dt)
    stage = dict(mode=mode, a=cast(a), b=cast(b), root=cast(root), transl=cast(transl), j_rest=cast(j_rest), obs=cast(joints_obs), conf=cast(conf),
                 rows=rows)
    timesteps = torch.linspace(sde.T, eps, sde.N).to(dt)
    n_run = sde.N - start_step if run_steps < 0 else run_steps
    x = x_mean = cast(x_init)
    trajs = []
    for k in range(n_run):
        i = start_step + k
        if forced is not None:
            x = cast(forced[k])
        vec_t = torch.ones(x.shape[0], dtype=dt) * timesteps[i]
        x, x_mean, _ = joint_guided_step(p, sde, x, vec_t, cast(noise[k, 0]), stage, norm=norm, grad_step=grad_step, **fw)
        x, x_mean = x.detach(), x_mean.detach()
        trajs.append(x)
    return torch.stack(trajs, 0), x, x_mean
