"""Float64 reference of the motion-denoising loop with PARTIAL 3D observations: per-(frame, joint) confidences and an observed-joint
list.  Test infrastructure, CPU only.

The loop is that of oracle/task_loops.motion_denoise_optimize (run/motion_denoising.py:199-300), restated around the same building
blocks -- score_ref.dposer_prior_loss, fk_torch.smplx_forward, smplify_normalize, gaussian_smoothing -- with the data term replaced
by the rule written out at dposer_motion_denoise_args (include/dposer_hip.h).  Per sequence of F frames, observed columns j:
    rows[j]: the tree joint column j observes (None: j);  c = conf[t, j] (None: 1);  an entry is LIVE iff c > 0 (false for NaN);
    a dead entry's observation is never read (it may be NaN) and its gradient is 0;
    r = J[t, rows[j]] - obs[t, j], s2 = |r|^2;  W = sum_live c;  N = sum_live c sqrt(max(s2, 1e-36)) (a NaN s2 stays NaN);
    data = N / W, KEPT iff W > 0 and data is finite and > 0;  d data / d J = (c / W) r / sqrt(s2) where live, kept and s2 > 1e-36.
With joints_conf = None and obs_joints = None this IS the oracle's loop (tests/test_md_partial_ref_cpu.py holds the two together).
tests/md_partial_cases.py holds the cases and the band; ``fault=`` seeds the defects a kernel could have.
"""
import numpy as np
import torch

from oracle import fk_torch
from oracle import score_ref as R
from oracle import task_loops as TL

# the faults ``motion_denoise_partial(fault=...)`` can seed into itself: tests/test_md_partial_ref_cpu.py shows that each one leaves the
# comparison band of tests/test_gpu_md_partial.py
FAULTS = ("conf_ignored",               # every entry live with c = 1, whatever the confidences say
          "mean_over_count",            # N divided by the entry count F n_obs instead of W (value and gradient)
          "grad_unweighted",            # the value weighted, the gradient rows of live entries all scaled 1 / W
          "nan_under_zero_poisons",     # dead entries multiplied by 0 instead of left out: 0 x NaN = NaN
          "rows_as_prefix",             # column j read as tree joint j, whatever the list says
          "blind_keeps_term")           # a sequence without a live entry falls back to the plain mean over all its entries


def data_term(joints, obs, conf, rows, fault=None):
    """The rule, for one sequence.  joints [F, >= max(rows) + 1, 3] (with gradient), obs [F, n_obs, 3], conf [F, n_obs] or None, rows: list
    or None.  Returns (data with its gradient path, or None when the term is dropped; the value to log: data when kept, 0 when dropped)."""
    F, n_obs = obs.shape[:2]
    idx = list(range(n_obs)) if rows is None or fault == "rows_as_prefix" else list(rows)
    c = torch.ones(F, n_obs, dtype=joints.dtype) if conf is None or fault == "conf_ignored" else conf
    live = c > 0
    if fault == "blind_keeps_term" and not bool(live.any()):
        c = torch.ones_like(c)
        live = c > 0
    zero = torch.zeros((), dtype=joints.dtype)
    cz = torch.where(live, c, zero)
    if fault == "nan_under_zero_poisons":
        r = joints[:, idx] - obs
    else:
        r = torch.where(live[..., None], joints[:, idx] - torch.where(live[..., None], obs, zero), zero)
    s2 = torch.sum(r * r, dim=2)
    dist = torch.sqrt(s2.clamp_min(1e-36))        # (torch's clamp keeps a NaN; its gradient is 0 below the bound)
    W = cz.sum()
    if fault == "mean_over_count":
        W = torch.tensor(float(F * n_obs), dtype=joints.dtype)
    if not bool(W > 0):
        return None, 0.0
    data = (cz * dist).sum() / W
    if fault == "grad_unweighted":
        plain = (torch.where(live, dist, zero)).sum() / W
        data = plain + (data - plain).detach()
    if not (bool(torch.isfinite(data)) and bool(data > 0)):
        return None, 0.0
    return data, data.detach()


def partial_metrics(obs, conf, rows, j_gt, j_out):
    """init_MPJPE [T]: the mean over the frame's live entries of |obs - gt joint| in cm (NaN without one); MPJPE_observed / MPJPE_unobserved
    [T]: the result's first 22 tree joints split by whether the joint has a live observation in that frame (NaN where the set is empty)."""
    T, n_obs = obs.shape[:2]
    idx = list(range(n_obs)) if rows is None else list(rows)
    live = np.ones((T, n_obs), dtype=bool) if conf is None else (np.asarray(conf) > 0)
    e0 = np.linalg.norm(np.where(live[..., None], np.asarray(obs), 0.0) - np.asarray(j_gt)[:, idx], axis=2)
    dist = np.linalg.norm(np.asarray(j_out)[:, :22] - np.asarray(j_gt)[:, :22], axis=2)
    seen = np.zeros((T, 22), dtype=bool)
    for col, row in enumerate(idx):
        if row < 22:
            seen[:, row] = live[:, col]
    mean = lambda x, m: np.array([x[t][m[t]].mean() * 100.0 if m[t].any() else np.nan for t in range(T)])
    return {"init_MPJPE": mean(e0, live), "MPJPE_observed": mean(dist, seen), "MPJPE_unobserved": mean(dist, ~seen)}


def motion_denoise_partial(p, sde, asset, mean, std, joints3d, gt_poses, init_poses, noise, *, joints_conf=None, obs_joints=None, iterations=5,
                           steps_per_iter=50, sample_trun=2.0, dposer_weight=1.0, dtype=torch.float64, norm_mode="zscore", rot6d=False,
                           time_strategy="3", sample_time=990, frames_per_sequence=None, fault=None, details=True):
    """oracle/task_loops.motion_denoise_optimize with the data term of partial observations.  joints3d [T, n_obs, 3], joints_conf [T, n_obs] or
    None, obs_joints: list of n_obs distinct tree joints or None.  Everything -- network, body model, pose leaf, Adam -- runs in ``dtype``:
    float64 is the arbiter, float32 sizes the reference's own rounding.  The other arguments and the ``details=True`` dict are the
    oracle's: pose, pose_steps, grad_steps, adam_m / adam_v, log [steps, S, 3], data_kept [steps, S], init_MPJPE / MPJPE / MPVPE [T] -- plus
    MPJPE_observed / MPJPE_unobserved [T] (``partial_metrics``; init_MPJPE is the live-entry mean)."""
    assert fault is None or fault in FAULTS, fault
    T = init_poses.shape[0]
    F = int(frames_per_sequence) if frames_per_sequence else T
    S = T // F
    assert S * F == T and F >= 2
    seqs = [slice(s * F, (s + 1) * F) for s in range(S)]
    norm_mode = norm_mode or "none"
    pd = {k: v.to(dtype) if v.is_floating_point() else v for k, v in p.items()}
    mean = None if norm_mode == "none" else torch.as_tensor(mean, dtype=dtype)
    std = None if norm_mode == "none" else torch.as_tensor(std, dtype=dtype)
    obs = torch.as_tensor(joints3d, dtype=dtype)
    conf = None if joints_conf is None else torch.as_tensor(joints_conf, dtype=dtype)
    rows = None if obs_joints is None else [int(j) for j in obs_joints]
    asset = {k: torch.as_tensor(v, dtype=dtype) if isinstance(v, np.ndarray) and v.dtype.kind == "f" else v for k, v in asset.items()}
    bm = lambda pose: fk_torch.smplx_forward(asset, pose.to(dtype), betas=None, dtype=dtype)
    with torch.no_grad():
        v_gt, j_gt = bm(torch.as_tensor(gt_poses, dtype=dtype))
    pose = torch.as_tensor(init_poses, dtype=dtype).clone().requires_grad_(True)
    opt = torch.optim.Adam([pose], 0.03, betas=(0.9, 0.999))
    ts = torch.linspace(1.0, 1e-3, sde.N)
    total = iterations * steps_per_iter
    z_all = torch.as_tensor(noise, dtype=dtype)
    log = torch.zeros(total, S, 3, dtype=dtype)
    kept = np.zeros((total, S), dtype=bool)
    pose_steps, grad_steps = [], []
    for it in range(iterations):
        for i in range(steps_per_iter):
            step = it * steps_per_iter + i
            opt.zero_grad()
            q = int(sample_time) if time_strategy == "2" else TL.quan_t_strategy3(step, total, sde.N, sample_trun)
            TL._smplify_check_label(sde, float(ts[q]))
            vec_t = torch.full((F,), float(ts[q]), dtype=dtype)
            x_n = TL.smplify_normalize(pose, rot6d, norm_mode, mean, std)
            x0 = x_n.detach()
            gprior = torch.zeros_like(x0)
            for s, sl in enumerate(seqs):
                l_prior, gprior[sl] = R.dposer_prior_loss(pd, sde, x0[sl], vec_t, z_all[step][sl], weighted=False, reduction="sum_over_batch",
                                                          batch_size=F)
                log[step, s, 2] = l_prior
            v, j = bm(pose)
            w_prior = 0.1 * (1 + it) * dposer_weight
            tots = []
            for s, sl in enumerate(seqs):
                temp = v[sl][:-1] - v[sl][1:]
                l_temp = torch.mean(torch.sqrt(torch.sum(temp * temp, dim=2)))
                tot = 10.0 * l_temp * (1 + it)
                l_data, logged = data_term(j[sl], obs[sl], None if conf is None else conf[sl], rows, fault)
                if l_data is not None:
                    tot = tot + 100.0 * l_data / (1 + it * it)
                kept[step, s] = l_data is not None
                log[step, s, 0], log[step, s, 1] = l_temp.detach(), logged
                tots.append(tot)
            tot = tots[0] if S == 1 else torch.stack(tots).sum()
            if rot6d:
                tot = tot + w_prior * (gprior * x_n).sum()
            tot.backward()
            if not rot6d:
                gp = gprior if norm_mode == "none" else (gprior / std if norm_mode == "zscore" else 2.0 * gprior / (std - mean))
                pose.grad += w_prior * gp
            grad_steps.append(pose.grad.detach().clone())
            opt.step()
            pose_steps.append(pose.detach().clone())
    final = pose.detach()
    smooth = final.clone()
    for sl in seqs:
        smooth[sl] = TL.gaussian_smoothing(final[sl], 3, 2.0)
        smooth[[sl.start, sl.stop - 1]] = final[[sl.start, sl.stop - 1]]
    with torch.no_grad():
        v, j = bm(smooth)
    je, ve = j[:, :22] - j_gt[:, :22], v - v_gt
    res = {"MPJPE": (torch.mean(torch.sqrt(torch.sum(je * je, dim=2)), dim=1) * 100.0).numpy(),
           "MPVPE": (torch.mean(torch.sqrt(torch.sum(ve * ve, dim=2)), dim=1) * 100.0).numpy()}
    res.update(partial_metrics(obs.numpy(), None if conf is None else conf.numpy(), rows, j_gt.numpy(), j.numpy()))
    if not details:
        return final.numpy(), res
    state = opt.state[pose]
    return dict(res, pose=final.numpy(), pose_steps=torch.stack(pose_steps).numpy(), grad_steps=torch.stack(grad_steps).numpy(),
                adam_m=state["exp_avg"].numpy(), adam_v=state["exp_avg_sq"].numpy(), log=log.numpy(), data_kept=kept)
