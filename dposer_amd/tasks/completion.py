"""Pose completion by optimisation under the DPoser prior -- counterpart of ``DPoserComp`` in the
reference's run/completion.py:95-207.

The whole optimisation loop is ONE call, ``dposer_completion_optimize``: the time-bias table of all 200 steps is built once,
the weights are packed once, and each step is perturb -> forward-only score network at the step's shared t -> one kernel for
the Tweedie estimate, the gradients of the weighted prior loss and of the masked MSE data term, and torch.optim.Adam's update
with per-sample moments.  The optimiser state is per sample, so the loop shards over GPUs with no collective
(``distributed.shard_bounds`` = the reference's DistributedEvalSampler arithmetic).  SDEs / models outside the fused path
(VE, Fourier embedding) run the same loop step by step through ``prior_loss`` and torch's Adam.
"""
import ctypes as C
import math

import numpy as np
import torch
from torch import nn

from .. import _C
from ..algorithms.advanced import sde_lib
from ..prior import prior_loss
from ._fused import ScoreNetCall, float_array


class DPoserComp:
    def __init__(self, diffusion_model, sde, continuous, batch_size=1):
        self.batch_size = batch_size
        self.sde = sde
        self.model = diffusion_model
        self.continuous = continuous
        self.data_loss = nn.MSELoss(reduction="mean")
        self._calls = 0

    def loss(self, x_0, t, weighted=False, z=None, multi_denoise=False):
        """completion.py:131-149 at one shared time ``t`` (python float): mean(weight * (x_0 - x0_hat)^2).  ``multi_denoise=True``: x0_hat
        from 10 DDIM steps down to t / 20 (completion.py:138) -- one ``dposer_prior_loss_multi`` call where ``prior_loss`` fuses it."""
        self._calls += 1
        return prior_loss(self.model, self.sde, x_0, t, weighted=bool(weighted), reduction="mean", z=z,
                          seed=self.model._rng_seed + 29, step=self._calls, continuous=bool(getattr(self, "continuous", True)),
                          **({"multi_denoise": 10} if multi_denoise else {}))      # (off: today's call, argument for argument)

    def get_loss_weights(self):
        """completion.py:151-155."""
        return {"data": lambda cst, it: 100 * cst / (1 + it), "dposer": lambda cst, it: 0.1 * cst * (it + 1)}

    @staticmethod
    def quan_t(step, total_steps, N, sample_trun=5.0):
        """time strategy '3' (completion.py:189-190); the reference multiplies an int64 tensor by a python float,
        i.e. in fp32."""
        return int(N - math.floor(float(np.float32(total_steps - step - 1) * np.float32(N / (sample_trun * total_steps)))) - 2)

    def _fused_supported(self):
        from ..algorithms.advanced.model import ScoreModelFC
        # (sub-VP: one score function; VE / VP: continuous or discrete, all on the fused kernels)
        return sde_lib.sde_desc(self.sde, bool(getattr(self, "continuous", True))) is not None and isinstance(self.model, ScoreModelFC)

    def _schedule(self, time_strategy, total_steps, sample_trun, sample_time):
        """quan_t of every step (completion.py:183-192)."""
        if time_strategy == "1":
            return [int(torch.randint(self.sde.N, [1])) for _ in range(total_steps)]
        if time_strategy == "2":
            return [int(sample_time)] * total_steps
        if time_strategy == "3":
            return [self.quan_t(step, total_steps, self.sde.N, sample_trun) for step in range(total_steps)]
        raise NotImplementedError("unsupported time sampling strategy")

    def optimize(self, observation, mask, time_strategy="3", lr=0.1, sample_trun=5.0, sample_time=900, iterations=2,
                 steps_per_iter=100, noise=None):
        """completion.py:167-207.  ``noise`` [total_steps, B, D]: injected z of the prior loss (tests)."""
        total_steps = iterations * steps_per_iter
        weights = self.get_loss_weights()
        timesteps = torch.linspace(self.sde.T, 1e-3, self.sde.N)          # host copy: t enters the kernels as a scalar
        quan = self._schedule(time_strategy, total_steps, sample_trun, sample_time)
        if self._fused_supported():
            _C.require_gpu(observation, "completion observation")
            model = self.model
            B, D = observation.shape
            net = ScoreNetCall(model, self.sde, bool(getattr(self, "continuous", True)), B, total_steps, observation.device)   # (packed once per loop)
            obs = observation.detach().contiguous().float()
            msk = mask.detach().contiguous().float()
            x = obs.clone()
            m, v = torch.zeros_like(x), torch.zeros_like(x)
            its = [s // steps_per_iter for s in range(total_steps)]
            t_host = float_array(timesteps[q] for q in quan)
            # the reference passes quan_t positionally into `weighted` (completion.py:196): weighted = bool(quan_t)
            wflag = (C.c_int32 * total_steps)(*[1 if q else 0 for q in quan])
            w_prior = float_array(weights["dposer"](1.0, it) for it in its)
            w_data = float_array(weights["data"](1.0, it) for it in its)
            nz = None if noise is None else noise.detach().contiguous().float()
            step0 = self._calls + 1
            self._calls += total_steps
            _C.check(net.eng.lib.dposer_completion_optimize(
                *net.head(), _C.ptr(x), _C.ptr(obs), _C.ptr(msk), _C.ptr(m), _C.ptr(v), t_host, wflag, w_prior, w_data, total_steps, float(lr),
                0.9, 0.999, 1e-8, _C.ptr(nz), int(model._rng_seed + 29), int(step0) & 0xFFFFFFFF, *net.tail(), B, _C.stream_ptr()),
                "dposer_completion_optimize")
            return observation * mask + x * (1.0 - mask)
        x = observation.clone().detach().requires_grad_(True)
        optimizer = torch.optim.Adam([x], lr, betas=(0.9, 0.999))
        for step, q in enumerate(quan):
            it = step // steps_per_iter
            optimizer.zero_grad()
            l_prior = self.loss(x, float(timesteps[q]), weighted=bool(q), z=None if noise is None else noise[step])
            l_data = self.data_loss(x * mask, observation * mask)
            tot = weights["dposer"](l_prior, it) + weights["data"](l_data, it)
            tot.backward()
            optimizer.step()
        return observation * mask + x.detach() * (1.0 - mask)


SOLVERS = ("dposer", "scoresde", "mcg", "dps", "dpm")


class _TaskArgs:
    """What the samplers read of run/demo.py's ``args``: the task name (sampling.py:416, 451)."""

    def __init__(self, task):
        self.task = task


def _completion_solver(solver, model, sde, continuous, shape, device, solver_kwargs):
    """``complete(observation, mask) -> completion`` for the diffusion solvers DPoser's completion table is compared against: ScoreSDE
    imputation (run/demo.py:389-394: get_sampling_fn's sampler with args.task == 'completion'), MCG and DPS (the loop over
    update_fn_guide, sampling.py:191-207: ``sampling.get_guided_sampler``).  The sampler's return value is the completion, unblended."""
    from ..algorithms.advanced import sampling
    kw = dict(solver_kwargs or {})
    eps = kw.pop("eps", 1e-3)
    extra = {k: kw.pop(k) for k in ("traj_stride", "seed") if k in kw}
    extra.setdefault("traj_stride", 0)               # the evaluation keeps no trajectory
    if solver == "scoresde":
        fn = sampling.get_pc_sampler(sde, shape, sampling.EulerMaruyamaPredictor, sampling.NoneCorrector, lambda v: v, snr=kw.pop("snr", 0.16),
                                     continuous=continuous, denoise=kw.pop("denoise", True), eps=eps, device=device, **kw)
        args = _TaskArgs("completion")
        return lambda observation, mask: fn(model, observation=observation, mask=mask, args=args, **extra)[1]
    if solver == "dpm":                              # the few-step solver: `steps` network evaluations per hypothesis
        fn = sampling.get_dpm_sampler(sde, shape, lambda v: v, steps=kw.pop("steps", 20), order=kw.pop("order", 2),
                                      skip_type=kw.pop("skip_type", "logSNR"), continuous=continuous, denoise=kw.pop("denoise", True), eps=eps,
                                      device=device, **kw)
        seed0, calls = extra.pop("seed", None), [0]

        def complete(observation, mask):             # a given seed keys the first call; every further call (hypothesis, batch) the next one
            calls[0] += 1
            return fn(model, observation=observation, mask=mask, seed=None if seed0 is None else int(seed0) + calls[0] - 1, **extra)[1]

        return complete
    fn = sampling.get_guided_sampler(sde, shape, lambda v: v, solver, continuous=continuous, eps=eps, device=device, **kw)
    return lambda observation, mask: fn(model, observation, mask, **extra)[1]


def evaluate_completion(model, sde, normalizer, body_model, poses, *, part="legs", hypo=1, batch_size=16384, continuous=True,
                        num_replicas=None, rank=None, optimize_kwargs=None, solver="dposer", solver_kwargs=None, fused_eval=False):
    """The evaluation loop of run/completion.py:215-323 (``inference``) for the poses of one test set, without its process / CLI
    shell: this rank's contiguous shard (DistributedEvalSampler arithmetic, EvaSampler.py:78-106) in batches of ``batch_size``
    with ``drop_last`` like the reference's DataLoader -> create_mask -> ``hypo`` completions -> de-normalise -> Evaler
    (min over hypotheses) -> mean of every metric over all samples of all ranks.

    Nothing synchronises with the host inside the loop: the per-sample metrics stay device tensors, and the end is ONE all-reduce
    of (sum, count) pairs (``distributed.reduce_metric_means``) instead of ``gather_object`` of every value (:300-305).
    ``poses`` [N, D] normalised test poses (the dataset's ``poses`` tensor); returns ``({metric: mean}, samples evaluated here)``.
    ``solver``: "dposer" (the optimisation above, ``optimize_kwargs``) or one of the diffusion samplers "scoresde" | "mcg" | "dps"
    (``solver_kwargs``: ``grad_step`` for MCG / DPS, ``eps``, ``denoise``, ``seed``) or the few-step "dpm" (DPM-Solver++:
    ``steps``, ``order``, ``skip_type``, ``eps``, ``seed``); each hypothesis is one sampler call, for "dpm" with its own seed.
    ``fused_eval``: score with ``Evaler.multi_eval_bodys(fused=True)`` -- one ``dposer_pose_pair_errors`` call per batch, no vertex tensors."""
    if solver not in SOLVERS:
        raise ValueError(f"unknown completion solver {solver!r}: expected one of {SOLVERS}")
    from .. import distributed as ddp
    from ..dataset.AMASS import Evaler
    from ..utils.misc import create_mask
    world = ddp.world_size() if num_replicas is None else num_replicas
    rk = ddp.rank() if rank is None else rank
    lo, hi = ddp.shard_bounds(poses.shape[0], world, rk)
    dev = next(model.parameters()).device
    evaler = Evaler(body_model=body_model, part=part)
    comp = DPoserComp(model, sde, continuous, batch_size=batch_size)      # one object: its call counter keys the in-kernel noise
    complete = None if solver == "dposer" else _completion_solver(solver, model, sde, continuous, (batch_size, poses.shape[1]), dev, solver_kwargs)
    results, done = [], 0
    for b0 in range(lo, hi - batch_size + 1, batch_size) if hi - lo >= batch_size else []:
        batch = poses[b0:b0 + batch_size].to(dev, non_blocking=True)
        mask, observation = create_mask(batch, part=part)
        if complete is None:
            outs = torch.stack([comp.optimize(observation, mask, **(optimize_kwargs or {})) for _ in range(hypo)], dim=1)
        else:
            outs = torch.stack([complete(observation, mask) for _ in range(hypo)], dim=1)
        preds = normalizer.offline_denormalize(outs, to_axis=True)
        gts = normalizer.offline_denormalize(batch, to_axis=True)
        results.append(evaler.multi_eval_bodys(preds, gts, as_tensors=True, fused=fused_eval))
        done += batch_size
    # fixed name list: a rank whose shard is shorter than one batch (drop_last) has no results to learn the names from
    return ddp.reduce_metric_means(results, device=dev, names=("mpjpe_body", "mpvpe_all")), done


def joint_residual_stage(body_model, normalizer, y0, joints3d, *, joints_conf=None, obs_joints=None, root_orient=None, trans=None, betas=None):
    """The measurement stage of guidance by observed 3D joints, for a batch of normalised poses: ``dposer_joint_guide_stage``, one library
    call.  ``y0`` [B, 63] normalised body poses (axis-angle networks only); ``joints3d`` [B, n_obs, 3]; ``joints_conf`` [B, n_obs] or
    [n_obs]-broadcastable (an entry counts iff its confidence is > 0; what lies under a dead entry may be NaN); ``obs_joints``: the n_obs
    distinct body joints in [0, 22) the columns observe (default 0 .. n_obs - 1); ``root_orient`` / ``trans`` [B, 3]; ``betas`` [B, n].
    Returns ``(s [B], v [B, 63])``: s = sum_live c |J(denormalise(y0)) - o|^2 and v = 1/2 ds/dy0 -- the chain rule over the joints alone
    (``dposer_fk_joints_backward``), no vertices.  Shapes and ``obs_joints`` are checked before any device work."""
    from ._fused import normalizer_tables
    from .motion_denoising import _partial_observation
    if y0.dim() != 2 or y0.shape[1] != 63:
        raise ValueError(f"y0 must be [B, 63] (21 axis-angle body joints; rot6d networks are not supported), got {list(y0.shape)}")
    B = int(y0.shape[0])
    if joints3d.dim() != 3 or joints3d.shape[0] != B or joints3d.shape[2] != 3 or not 1 <= joints3d.shape[1] <= 22:
        raise ValueError(f"joints3d must be [{B}, 1..22, 3], got {list(joints3d.shape)}")
    for name, t in (("root_orient", root_orient), ("trans", trans)):
        if t is not None and tuple(t.shape) != (B, 3):
            raise ValueError(f"{name} must be [{B}, 3], got {list(t.shape)}")
    conf, rows = _partial_observation(joints3d, joints_conf, obs_joints, 22)
    _C.require_gpu(y0, "y0")
    dev = y0.device
    core = body_model.bm
    with torch.no_grad():
        _, j_rest, batched = core.rest_shape(betas, None)
    f32 = lambda t: None if t is None else t.detach().to(dev).contiguous().float()
    y, obs, root, tr, jr = f32(y0), f32(joints3d), f32(root_orient), f32(trans), f32(j_rest)
    mode, na, nb = normalizer_tables(normalizer, y)
    rows_d = None if rows is None else torch.tensor(rows, dtype=torch.int32, device=dev)
    lib = _C.lib()
    s = torch.empty(B, dtype=torch.float32, device=dev)
    v = torch.empty(B, 63, dtype=torch.float32, device=dev)
    scratch = torch.empty(lib.dposer_joint_guide_stage_scratch_bytes(B), dtype=torch.uint8, device=dev)
    _C.check(lib.dposer_joint_guide_stage(core._handle(), _C.ptr(y), 63, mode, _C.ptr(na), _C.ptr(nb), _C.ptr(root), _C.ptr(tr), _C.ptr(jr),
                                          1 if batched else 0, _C.ptr(obs), _C.ptr(conf), _C.ptr(rows_d), int(obs.shape[1]), _C.ptr(s), _C.ptr(v),
                                          _C.ptr(scratch), B, _C.stream_ptr()), "dposer_joint_guide_stage")
    return s, v


def sample_from_joints(model, sde, normalizer, body_model, joints3d, *, joints_conf=None, obs_joints=None, hypo=1, grad_step=1.0, norm="sample",
                       gt_poses=None, root_orient=None, trans=None, betas=None, continuous=True, eps=1e-3, noise=None, seed=None, z=None, start_step=0):
    """``hypo`` plausible bodies for every set of observed 3D joints: DPS under the DPoser prior with the posed joints as the measurement
    (``sampling.get_joint_guided_sampler``), all hypotheses in one batch -- what ``evaluate_completion(hypo=K)`` does for masked poses.

    ``joints3d`` [B, n_obs, 3] (NaN allowed under a confidence that is not > 0: ``utils.misc.occlude_joints`` makes such inputs),
    ``joints_conf`` [B, n_obs] or None, ``obs_joints`` the observed tree joints (default 0 .. n_obs - 1); ``root_orient`` / ``trans`` [B, 3],
    ``betas`` [B, n].  The observation is tiled over the hypotheses (rows b * hypo + k); ``noise`` [N - start_step, 1, B * hypo, 63] / ``z`` [B * hypo, 63]
    inject the draws and ``start_step`` enters the loop late (``z`` is then the state at that index).  Returns a dict: ``poses`` [B, hypo, 63] axis-angle (de-normalised), ``joint_error`` [B, hypo] the mean distance in
    metres between the posed and the observed joints over the live entries (NaN for a sample without one) and, with ``gt_poses``
    [B, 63], ``mpjpe`` / ``mpvpe`` [B]: the minimum over the hypotheses through ``utils.metric.pose_pair_errors``."""
    from ..algorithms.advanced import sampling
    from ..utils.metric import pose_pair_errors
    from .motion_denoising import _partial_observation
    if joints3d.dim() != 3 or joints3d.shape[2] != 3:
        raise ValueError(f"joints3d must be [B, n_obs, 3], got {list(joints3d.shape)}")
    if int(hypo) < 1:
        raise ValueError(f"hypo must be >= 1, got {hypo}")
    B, K = int(joints3d.shape[0]), int(hypo)
    conf, rows = _partial_observation(joints3d, joints_conf, obs_joints, 22)          # (host checks before any device work)
    if gt_poses is not None and tuple(gt_poses.shape) != (B, 63):
        raise ValueError(f"gt_poses must be [{B}, 63], got {list(gt_poses.shape)}")
    tile = lambda t: None if t is None else t.repeat_interleave(K, dim=0)
    dev = joints3d.device
    fn = sampling.get_joint_guided_sampler(sde, (B * K, 63), body_model, normalizer, grad_step=grad_step, norm=norm, continuous=continuous,
                                           denoise=True, eps=eps, device=dev)
    obs_t, conf_t, root_t, tr_t, betas_t = tile(joints3d), tile(conf), tile(root_orient), tile(trans), tile(betas)
    _, x = fn(model, obs_t, conf_t, rows, root_t, tr_t, betas_t, z=z, start_step=start_step, traj_stride=0, noise=noise, seed=seed)
    with torch.no_grad():
        poses = normalizer.offline_denormalize(x)
        joints = body_model.fk_joints(poses, root_orient=root_t, trans=tr_t, betas=betas_t)
        idx = torch.arange(obs_t.shape[1], device=dev) if rows is None else torch.tensor(rows, dtype=torch.long, device=dev)
        live = torch.ones(obs_t.shape[:2], dtype=torch.bool, device=dev) if conf_t is None else conf_t > 0
        d = joints[:, idx] - torch.where(live[..., None], obs_t.float(), torch.zeros_like(obs_t, dtype=torch.float32))
        dist = torch.where(live, torch.sqrt((d * d).sum(dim=2)), torch.zeros_like(d[..., 0]))
        cnt = live.sum(dim=1)
        err = torch.where(cnt > 0, dist.sum(dim=1) / cnt.clamp_min(1), torch.full_like(dist[:, 0], float("nan")))
        out = {"poses": poses.reshape(B, K, 63), "joint_error": err.reshape(B, K)}
        if gt_poses is not None:
            pe = pose_pair_errors(body_model, gt_poses.to(dev).float(), out["poses"], betas=betas)
            out["mpjpe"], out["mpvpe"] = pe["mpjpe"], pe["mpvpe"]
    return out


def keypoint_residual_stage(body_model, normalizer, y0, keypoints2d, *, keypoints_conf=None, obs_joints=None, cam_t, camera_center, focal_length=5000.0,
                            sigma=100.0, z_near=0.1, root_orient=None, betas=None):
    """The measurement stage of guidance by observed 2D keypoints, for a batch of normalised poses: ``dposer_keypoint_guide_stage``, one
    library call.  ``y0`` [B, 63] normalised body poses (axis-angle networks only); ``keypoints2d`` [B, n_obs, 2] pixels; ``keypoints_conf``
    [B, n_obs] or [n_obs]; ``obs_joints``: the n_obs distinct body joints in [0, 22) the columns observe (default 0 .. n_obs - 1);
    ``cam_t`` [B, 3] the camera translation (added to the posed joints, SMPLify's ``transl=camera_t``), ``camera_center`` [B, 2],
    ``focal_length`` a number or [B]; ``root_orient`` [B, 3]; ``betas`` [B, n].  An entry counts iff its confidence is > 0 and its joint's
    depth is > ``z_near``; what lies under a dead entry may be NaN.  Returns ``(s [B], v [B, 63])``: s = sum_live c^2 (rho(ru) + rho(rv)),
    r = focal J_xy / J_z - (k - centre), rho the Geman-McClure function of ``sigma`` (<= 0: r^2), and v = 1/2 ds/dy0.  Shapes, ``obs_joints``
    and the scalars are checked before any device work."""
    from ..algorithms.advanced.sampling import _keypoint_guided_problem
    from ._fused import normalizer_tables
    if y0.dim() != 2 or y0.shape[1] != 63:
        raise ValueError(f"y0 must be [B, 63] (21 axis-angle body joints; rot6d networks are not supported), got {list(y0.shape)}")
    B = int(y0.shape[0])
    kp, conf, rows, focal = _keypoint_guided_problem(keypoints2d, keypoints_conf, obs_joints, cam_t, camera_center, focal_length, sigma, z_near, root_orient,
                                                     betas, B)
    _C.require_gpu(y0, "y0")
    dev = y0.device
    core = body_model.bm
    with torch.no_grad():
        _, j_rest, batched = core.rest_shape(betas, None)
    f32 = lambda t: None if t is None else t.detach().to(dev).contiguous().float()
    y, kp, conf, root, tr, jr, fo, ce = f32(y0), f32(kp), f32(conf), f32(root_orient), f32(cam_t), f32(j_rest), f32(focal), f32(camera_center)
    mode, na, nb = normalizer_tables(normalizer, y)
    rows_d = None if rows is None else torch.tensor(rows, dtype=torch.int32, device=dev)
    lib = _C.lib()
    s = torch.empty(B, dtype=torch.float32, device=dev)
    v = torch.empty(B, 63, dtype=torch.float32, device=dev)
    scratch = torch.empty(lib.dposer_keypoint_guide_stage_scratch_bytes(B), dtype=torch.uint8, device=dev)
    _C.check(lib.dposer_keypoint_guide_stage(core._handle(), _C.ptr(y), 63, mode, _C.ptr(na), _C.ptr(nb), _C.ptr(root), _C.ptr(tr), _C.ptr(jr),
                                             1 if batched else 0, _C.ptr(kp), _C.ptr(conf), _C.ptr(rows_d), int(kp.shape[1]), _C.ptr(fo), _C.ptr(ce),
                                             float(sigma), float(z_near), _C.ptr(s), _C.ptr(v), _C.ptr(scratch), B, _C.stream_ptr()),
             "dposer_keypoint_guide_stage")
    return s, v


def sample_from_keypoints(model, sde, normalizer, body_model, keypoints2d, *, keypoints_conf=None, obs_joints=None, cam_t, camera_center,
                          focal_length=5000.0, sigma=100.0, z_near=0.1, hypo=1, grad_step=1.0, norm="sample", gt_poses=None, root_orient=None, betas=None,
                          continuous=True, eps=1e-3, noise=None, seed=None, z=None, start_step=0):
    """``hypo`` plausible bodies for every set of observed 2D keypoints: DPS under the DPoser prior with the reprojected joints as the
    measurement (``sampling.get_keypoint_guided_sampler``), all hypotheses in one batch.  Where SMPLify returns one body per image, this
    returns several that reproject onto the same keypoints and differ in what one view leaves open.

    ``keypoints2d`` [B, n_obs, 2] pixels (NaN allowed under a confidence that is not > 0), ``keypoints_conf`` [B, n_obs] or None,
    ``obs_joints`` the observed tree joints in [0, 22) (default 0 .. n_obs - 1); ``cam_t`` [B, 3], ``camera_center`` [B, 2],
    ``focal_length`` a number or [B]; ``root_orient`` [B, 3], ``betas`` [B, n].  The observation is tiled over the hypotheses (rows
    b * hypo + k); ``noise`` [N - start_step, 1, B * hypo, 63] / ``z`` [B * hypo, 63] inject the draws and ``start_step`` enters the loop
    late.  Returns a dict: ``poses`` [B, hypo, 63] axis-angle (de-normalised); ``reprojection_error`` [B, hypo]: the mean pixel distance
    between the projected and the observed keypoints over the entries live at the final pose (confidence > 0 and depth > ``z_near``),
    without the robustifier, NaN where there are none; ``depth_spread`` [B]: the standard deviation over the hypotheses of the mean depth
    of the 22 joints, in metres (0 for ``hypo`` = 1) -- what a sampler shows and an optimiser cannot; and, with ``gt_poses`` [B, 63],
    ``mpjpe`` / ``mpvpe`` [B]: the minimum over the hypotheses through ``utils.metric.pose_pair_errors``."""
    from ..algorithms.advanced import sampling
    from ..utils.metric import pose_pair_errors
    if keypoints2d.dim() != 3 or keypoints2d.shape[2] != 2:
        raise ValueError(f"keypoints2d must be [B, n_obs, 2], got {list(keypoints2d.shape)}")
    if int(hypo) < 1:
        raise ValueError(f"hypo must be >= 1, got {hypo}")
    B, K = int(keypoints2d.shape[0]), int(hypo)
    kp, conf, rows, focal = sampling._keypoint_guided_problem(keypoints2d, keypoints_conf, obs_joints, cam_t, camera_center, focal_length, sigma, z_near,
                                                              root_orient, betas, B)                  # (host checks before any device work)
    if gt_poses is not None and tuple(gt_poses.shape) != (B, 63):
        raise ValueError(f"gt_poses must be [{B}, 63], got {list(gt_poses.shape)}")
    tile = lambda t: None if t is None else t.repeat_interleave(K, dim=0)
    dev = keypoints2d.device
    fn = sampling.get_keypoint_guided_sampler(sde, (B * K, 63), body_model, normalizer, focal_length=tile(focal), sigma=sigma, z_near=z_near,
                                              grad_step=grad_step, norm=norm, continuous=continuous, denoise=True, eps=eps, device=dev)
    kp_t, conf_t, root_t, cam_tt, cen_t, betas_t, focal_t = tile(kp), tile(conf), tile(root_orient), tile(cam_t), tile(camera_center), tile(betas), tile(focal)
    _, x = fn(model, kp_t, conf_t, rows, cam_t=cam_tt, camera_center=cen_t, root_orient=root_t, betas=betas_t, z=z, start_step=start_step, traj_stride=0,
              noise=noise, seed=seed)
    with torch.no_grad():
        poses = normalizer.offline_denormalize(x)
        joints = body_model.fk_joints(poses, root_orient=root_t, trans=cam_tt.to(dev).float(), betas=betas_t)[:, :22]
        idx = torch.arange(kp_t.shape[1], device=dev) if rows is None else torch.tensor(rows, dtype=torch.long, device=dev)
        P = joints[:, idx]
        live = (torch.ones(kp_t.shape[:2], dtype=torch.bool, device=dev) if conf_t is None else conf_t > 0) & (P[..., 2] > z_near)
        Zs = torch.where(live, P[..., 2], torch.ones_like(P[..., 2]))
        proj = focal_t.to(dev)[:, None, None] * (P[..., :2] / Zs[..., None]) + cen_t.to(dev).float()[:, None, :]
        d = proj - torch.where(live[..., None], kp_t.float(), torch.zeros_like(kp_t, dtype=torch.float32))
        dist = torch.where(live, torch.sqrt((d * d).sum(dim=2)), torch.zeros_like(d[..., 0]))
        cnt = live.sum(dim=1)
        err = torch.where(cnt > 0, dist.sum(dim=1) / cnt.clamp_min(1), torch.full_like(dist[:, 0], float("nan")))
        depth = joints[..., 2].mean(dim=1).reshape(B, K)
        out = {"poses": poses.reshape(B, K, 63), "reprojection_error": err.reshape(B, K), "depth_spread": depth.std(dim=1, unbiased=False)}
        if gt_poses is not None:
            pe = pose_pair_errors(body_model, gt_poses.to(dev).float(), out["poses"], betas=betas)
            out["mpjpe"], out["mpvpe"] = pe["mpjpe"], pe["mpvpe"]
    return out
