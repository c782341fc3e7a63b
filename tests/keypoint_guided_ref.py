"""The float64 rule of the keypoint-residual stage (dposer_keypoint_guide_stage) and of DPS on observed 2D keypoints
(dposer_keypoint_guided_sampler).  TEST INFRASTRUCTURE: the chain, the normaliser and the confidence rule are those of
tests/joint_guided_ref.py; the camera is the reference's perspective_projection with the identity rotation, the residual its gmof
weighted by the squared confidence (lib/body_model/fitting_losses.py:6-47,69-75), written in the order the library's contract fixes:
the centre is taken off the observation, r = focal (X / Z) - (k - centre)."""
import torch

from joint_guided_ref import denormalise, fk22

__all__ = ["reprojection_terms", "live_entries", "stage_terms", "stage_sum", "keypoint_stage", "keypoint_guided_step", "keypoint_guided_loop"]


def reprojection_terms(joints, keypoints, focal, center, sigma):
    """c-free per-entry terms [B, n, 2] -> summed over (u, v): rho(ru) + rho(rv) [B, n] for posed ``joints`` [B, n, 3]; ``focal`` [B],
    ``center`` [B, 2]; sigma <= 0: no robustifier."""
    r = focal[:, None, None] * (joints[..., :2] / joints[..., 2:3]) - (keypoints - center[:, None, :])
    r2 = r * r
    rho = (sigma ** 2 * r2) / (sigma ** 2 + r2) if sigma > 0 else r2
    return rho.sum(dim=2)


def live_entries(Z, keypoints, conf, z_near):
    """(live [B, n_obs] bool, c with zeros where dead, keypoints with zeros where dead): live iff c > 0 (false for 0, negatives and NaN)
    and Z > z_near; what lies under a dead entry never enters a sum."""
    c = torch.ones_like(Z) if conf is None else conf.to(Z.dtype)
    live = (c > 0) & (Z.detach() > z_near)
    return live, torch.where(live, c, torch.zeros_like(c)), torch.where(live[..., None], keypoints, torch.zeros_like(keypoints))


def stage_terms(y0, mode, a, b, root, transl, j_rest, kp, conf, rows, focal, center, sigma, z_near):
    """(per-entry c^2 (rho(ru) + rho(rv)) [B, n_obs] with zeros where dead, live [B, n_obs], posed joints [B, 22, 3])."""
    J = fk22(denormalise(y0, mode, a, b), root, j_rest, transl)
    idx = list(range(kp.shape[1])) if rows is None else [int(r) for r in rows]
    P = J[:, idx]
    live, c, k = live_entries(P[..., 2], kp, conf, z_near)
    safe = torch.where(live[..., None], P, torch.ones_like(P))                   # a dead entry's joint (Z <= z_near, maybe 0) is not divided by
    terms = c * c * reprojection_terms(safe, k, focal, center, sigma)
    return torch.where(live, terms, torch.zeros_like(terms)), live, J


def stage_sum(y0, **kw):
    """s[b] = sum_live c^2 (rho(ru) + rho(rv)), differentiable in y0; every tensor in y0's dtype."""
    return stage_terms(y0, **kw)[0].sum(dim=1)


def keypoint_stage(y0, **kw):
    """(s [B], v [B, 63] = 1/2 ds/dy0, live [B, n_obs]) by autograd, in the dtype of ``y0``."""
    y = y0.detach().clone().requires_grad_(True)
    terms, live, _ = stage_terms(y, **kw)
    s = terms.sum(dim=1)
    (g,) = torch.autograd.grad(s.sum(), [y])
    return s.detach(), 0.5 * g, live


def keypoint_guided_step(p, sde, x_t, t, z, stage, *, norm, grad_step, group=None, score_shift=None, **fw):
    """One index of DPS on observed 2D keypoints: joint_guided_ref.joint_guided_step with this module's ``stage_sum``.  ``stage``: the
    keyword arguments of ``stage_sum`` behind y0, in the dtype of ``x_t``.  ``score_shift`` [rows, D]: a constant added to the network's
    output -- the rule stepped on ANOTHER forward's values (the Jacobian stays the rule's own): with shift = a library forward minus the
    rule's, what that forward's error alone does to the step.  Returns (x', y_mean, s, min Z over the 22 joints of y0)."""
    import numpy as np
    from oracle import score_ref as R
    x = x_t.detach().clone().requires_grad_(True)
    dt = -1.0 / sde.N
    drift, g, score = R.rsde_sde(p, sde, x, t, **fw)
    if score_shift is not None:
        score = score + score_shift
        drift = drift - g[:, None] ** 2 * score_shift
    alpha, sigma = sde.alpha_sigma(t)
    y_mean = x.detach() + drift.detach() * dt
    y_hat = y_mean + g[:, None] * np.sqrt(-dt) * z
    y0 = (x + (sigma ** 2)[:, None] * score) / alpha
    terms, _, J = stage_terms(y0, **stage)
    s = terms.sum(dim=1)
    sn = s.reshape(-1, group or s.shape[0]).sum(dim=1) if norm == "batch" else s
    on = sn > 0
    total = torch.where(on, torch.sqrt(torch.where(on, sn, torch.ones_like(sn))), torch.zeros_like(sn)).sum()
    grad = torch.autograd.grad(total, x)[0] if bool(on.any()) else torch.zeros_like(y_hat)
    bad = ~torch.isfinite(sn)
    if bool(bad.any()):                              # a NaN / Inf keypoint under a positive confidence: its norm's rows are not finite
        rows_bad = bad.repeat_interleave(group or s.shape[0]) if norm == "batch" else bad
        grad = torch.where(rows_bad[:, None], torch.full_like(grad, float("nan")), grad)
    return (y_hat - grad_step * grad).detach(), y_mean, s.detach(), float(J[..., 2].detach().min())


def keypoint_guided_loop(p, sde, x_init, noise, stage, *, norm="sample", grad_step=1.0, eps=1e-3, start_step=0, run_steps=-1, dtype=None, **fw):
    """joint_guided_ref.joint_guided_loop over ``keypoint_guided_step``; ``stage``: ``stage_sum``'s keyword arguments (cast here).
    Returns (trajs [n, B, D], x, x_mean, min Z over the run)."""
    from guided_ref import params_as
    dt = dtype or x_init.dtype
    cast = lambda v: v.to(dt) if torch.is_tensor(v) and v.is_floating_point() else v
    p = params_as(p, dt)
    stage = {k: cast(v) for k, v in stage.items()}
    timesteps = torch.linspace(sde.T, eps, sde.N).to(dt)
    n_run = sde.N - start_step if run_steps < 0 else run_steps
    x = x_mean = x_init.to(dt)
    trajs, zmin = [], float("inf")
    for k in range(n_run):
        vec_t = torch.ones(x.shape[0], dtype=dt) * timesteps[start_step + k]
        x, x_mean, _, zm = keypoint_guided_step(p, sde, x, vec_t, torch.as_tensor(noise[k, 0]).to(dt), stage, norm=norm, grad_step=grad_step, **fw)
        x, x_mean = x.detach(), x_mean.detach()
        zmin = min(zmin, zm)
        trajs.append(x)
    return torch.stack(trajs, 0), x, x_mean, zmin
