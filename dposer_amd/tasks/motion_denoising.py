"""Motion denoising: DPoser prior + SMPL-X FK/LBS fitting of noisy 3D joints -- counterpart of
``MotionDenoise`` in the reference's run/motion_denoising.py:63-300.

Per Adam step: z-score normalise -> ``dposer_prior_loss`` -> ``BodyModel`` forward WITH gradient
(dposer_lbs_forward / dposer_lbs_backward) -> temporal term on vertices + data term on Jtr[:, :22].
The frames of one sequence are coupled by the temporal term, so data parallelism is over sequences.

The whole loop is ONE call, ``dposer_motion_denoise_optimize`` (axis-angle or 6-D rotation representation, sub-VP / VP SDE, positional or Fourier time embedding):
all steps are queued from C, the loss gradients and torch.optim.Adam's update are kernels, nothing returns to the host in
between.  Other configurations (and ``fused=False``) run the same step through autograd and torch's Adam.

Partial observations (no counterpart in the reference): ``joints_conf=`` gives every (frame, joint) entry a confidence and ``obs_joints=``
names the tree joints the columns of ``joints3d`` observe -- occluded limbs (``utils.misc.occlude_joints``), dropped detections, sparse
trackers.  The rule is written out at ``dposer_motion_denoise_args`` in include/dposer_hip.h; both paths apply it.

``optimize(..., vis=True)`` writes what the reference writes into ``out_path`` (motion_denoising.py:204-207,287-290): the skeleton frames
of the noisy joints, the ground-truth and result body renders, the three-panel merged frames and the motion video -- each through one
batched call (``vis_skeletons``, ``MotionDenoise.visualize``, ``seq_to_video``).
"""
import ctypes as C
import math
import os

import numpy as np
import torch

from .. import _C
from ..algorithms.advanced import sde_lib
from ..prior import prior_loss, red_diff
from ..utils.misc import gaussian_smoothing
from ._fused import BodyTables, ScoreNetCall, float_array, normalizer_tables


def _axis_angle_to_rot6d_autograd(aa):
    """Differentiable axis-angle -> 6-D (first two columns of the rotation matrix, row-major: lib/utils/transforms.py:238-255) for the
    step-by-step loop with rot_rep = 'rot6d' -- the HIP conversion kernel has no backward.  Rodrigues as smplx writes it
    (angle = ||r + 1e-8||), i.e. what the one-call loop's kernels evaluate."""
    angle = torch.norm(aa + 1e-8, dim=1, keepdim=True)
    k = aa / angle
    s, c = torch.sin(angle), torch.cos(angle)
    kx, ky, kz = k[:, 0:1], k[:, 1:2], k[:, 2:3]
    c1 = 1.0 - c
    R00 = 1.0 + c1 * (-(kz * kz) - ky * ky)
    R01 = s * (-kz) + c1 * (kx * ky)
    R10 = s * kz + c1 * (kx * ky)
    R11 = 1.0 + c1 * (-(kz * kz) - kx * kx)
    R20 = s * (-ky) + c1 * (kx * kz)
    R21 = s * kx + c1 * (ky * kz)
    return torch.cat([R00, R01, R10, R11, R20, R21], dim=1)


def _normalize_with_grad(nz, pose):
    """Posenormalizer.offline_normalize(pose, from_axis=True) with a gradient path to the axis-angle pose also for rot_rep = 'rot6d'."""
    if getattr(nz, "rot_rep", "axis") != "rot6d":
        return nz.offline_normalize(pose, from_axis=True)
    six = _axis_angle_to_rot6d_autograd(pose.reshape(-1, 3)).reshape(*pose.shape[:-1], -1)
    return nz.offline_normalize(six, from_axis=False)


def _partial_observation(joints3d, joints_conf, obs_joints, n_tree):
    """Host checks of the two partial-observation arguments (the rule: include/dposer_hip.h, dposer_motion_denoise_args).
    ``joints3d`` [F, n_obs, 3] or [S, F, n_obs, 3]; ``obs_joints``: n_obs distinct tree joints in [0, n_tree); ``joints_conf``:
    [F, n_obs] (shared by every sequence) or joints3d's own leading shape.  Returns (float32 confidences shaped like joints3d without
    its last axis, or None; the joint list, or None)."""
    n_obs = int(joints3d.shape[-2])
    rows = None
    if obs_joints is not None:
        rows = [int(j) for j in (obs_joints.tolist() if torch.is_tensor(obs_joints) else obs_joints)]
        if len(rows) != n_obs:
            raise ValueError(f"obs_joints names {len(rows)} joints, joints3d observes {n_obs}")
        if any(j < 0 or j >= n_tree for j in rows):
            raise ValueError(f"obs_joints must be tree joints in [0, {n_tree}), got {rows}")
        if len(set(rows)) != len(rows):
            raise ValueError(f"obs_joints must be distinct, got {rows}")
    conf = None
    if joints_conf is not None:
        conf = torch.as_tensor(joints_conf, device=joints3d.device).float()
        lead = tuple(joints3d.shape[:-1])
        if tuple(conf.shape) not in (lead, lead[-2:]):
            raise ValueError(f"joints_conf must be {list(lead[-2:])}" + (f" or {list(lead)}" if len(lead) > 2 else "") + f", got {list(conf.shape)}")
        conf = conf.expand(lead).contiguous()
    return conf, rows


def _partial_metrics(obs, conf, rows, gt_joints, out_joints):
    """The metrics that depend on what was observed, per frame in cm: ``init_MPJPE`` = the mean over the frame's live entries of
    |obs - gt joint| (NaN for a frame without one), ``MPJPE_observed`` / ``MPJPE_unobserved`` = the result's first 22 tree joints split by
    whether the joint has a live observation in that frame (NaN where the set is empty).  obs [T, n_obs, 3], conf [T, n_obs] or None,
    rows list or None, gt_joints / out_joints [T, >= 22 (and every row of ``rows``), 3]."""
    T, n_obs = obs.shape[:2]
    idx = torch.arange(n_obs, device=obs.device) if rows is None else torch.tensor(rows, dtype=torch.long, device=obs.device)
    live = torch.ones(T, n_obs, dtype=torch.bool, device=obs.device) if conf is None else conf > 0
    nan = torch.full((T,), float("nan"), dtype=obs.dtype, device=obs.device)

    def masked_mean(x, m):
        cnt = m.sum(dim=1)
        return torch.where(cnt > 0, torch.where(m, x, torch.zeros_like(x)).sum(dim=1) / cnt.clamp_min(1), nan) * 100.0

    e0 = torch.where(live[..., None], obs, gt_joints[:, idx]) - gt_joints[:, idx]
    seen = torch.zeros(T, 22, dtype=torch.bool, device=obs.device)
    body = idx < 22
    seen[:, idx[body]] = live[:, body]
    je = out_joints[:, :22] - gt_joints[:, :22]
    dist = torch.sqrt(torch.sum(je * je, dim=2))
    return {"init_MPJPE": masked_mean(torch.sqrt(torch.sum(e0 * e0, dim=2)), live), "MPJPE_observed": masked_mean(dist, seen),
            "MPJPE_unobserved": masked_mean(dist, ~seen)}


# the canvas and camera of run/motion_denoising.py:30-32 (``visualize`` renders over a white 512 x 384 canvas)
VIS_CANVAS = (512, 384)
VIS_FOCAL = (1500, 1500)
VIS_PRINCPT = (200, 192)


class MotionDenoise:
    def __init__(self, config, args, diffusion_model, body_model, sde_N=1000, dposer_weight=1.0, out_path=None, debug=False,
                 batch_size=1, normalizer=None):
        from ..dataset.AMASS import Posenormalizer
        self.args, self.debug, self.device = args, debug, args.device
        self.body_model = body_model
        self.dposer_weight = dposer_weight
        self.out_path = out_path
        self.batch_size = batch_size
        self.betas = torch.zeros((batch_size, 10), device=self.device)
        self.poses = torch.randn((batch_size, 63), device=self.device) * 0.01
        self.Normalizer = normalizer if normalizer is not None else Posenormalizer(
            data_path=f"{args.dataset_folder}/{args.version}/train", normalize=config.data.normalize, min_max=config.data.min_max,
            rot_rep=config.data.rot_rep, device=args.device)
        name = config.training.sde.lower()
        if name == "vpsde":
            sde = sde_lib.VPSDE(beta_min=config.model.beta_min, beta_max=config.model.beta_max, N=config.model.num_scales)
        elif name == "subvpsde":
            sde = sde_lib.subVPSDE(beta_min=config.model.beta_min, beta_max=config.model.beta_max, N=config.model.num_scales)
        elif name == "vesde":
            sde = sde_lib.VESDE(sigma_min=config.model.sigma_min, sigma_max=config.model.sigma_max, N=config.model.num_scales)
        else:
            raise NotImplementedError(f"SDE {config.training.sde} unknown.")
        sde.N = sde_N
        self.sde = sde
        self.continuous = bool(getattr(config.training, "continuous", True))      # motion_denoising.py:94: the score function's flavour
        self.model = diffusion_model
        self._calls = 0

    def DPoser_loss(self, x_0, t, weighted=False, z=None, multi_denoise=False):
        """motion_denoising.py:124-143: sum(weight * (x_0 - x0_hat)^2) / batch_size.  ``multi_denoise=True``: x0_hat from 10 DDIM steps
        down to t / 20 (:132) -- one ``dposer_prior_loss_multi`` call where ``prior_loss`` fuses it."""
        self._calls += 1
        return prior_loss(self.model, self.sde, x_0, t, weighted=weighted, reduction="sum_over_batch", batch_size=self.batch_size, z=z,
                          seed=self.model._rng_seed + 31, step=self._calls, continuous=getattr(self, "continuous", True),
                          **({"multi_denoise": 10} if multi_denoise else {}))      # (off: today's call, argument for argument)

    def RED_Diff(self, x_0, t, z=None):
        """motion_denoising.py:145-154: mean_b(sigma / alpha * <(eps_pred - z).detach(), x_0>) at one shared time ``t`` -- one
        ``dposer_prior_red_diff`` call where ``red_diff`` fuses it."""
        self._calls += 1
        return red_diff(self.model, self.sde, x_0, t, z=z, seed=self.model._rng_seed + 31, step=self._calls,
                        continuous=getattr(self, "continuous", True))

    def get_loss_weights(self):
        """motion_denoising.py:157-163."""
        return {"temp": lambda cst, it: 10.0 ** 1 * cst * (1 + it), "data": lambda cst, it: 10.0 ** 2 * cst / (1 + it * it),
                "dposer": lambda cst, it: 10.0 ** -1 * cst * (1 + it) * self.dposer_weight}

    def _fused_supported(self):
        from ..algorithms.advanced.model import ScoreModelFC
        from ..body_model.body_model import BodyModel
        nz = self.Normalizer
        return (sde_lib.sde_desc(self.sde, bool(getattr(self, "continuous", True))) is not None and isinstance(self.model, ScoreModelFC)
                and isinstance(self.body_model, BodyModel)
                and getattr(nz, "rot_rep", None) in ("axis", "rot6d") and self.batch_size >= 2)

    def _optimize_fused(self, pose, init_joints, t_list, its, weights, noise, frames_per_sequence=0, betas=None, conf=None, obs_rows=None):
        """All optimisation steps in one C call; ``pose`` [T, 63] is updated in place (T = sequences x frames_per_sequence when a
        batch of sequences is advanced together).  Returns the per-step loss log [steps, sequences, 3] (temp, data, prior).
        ``conf`` [T, n_obs] / ``obs_rows`` (joint list): partial observations; both None = the complete, equally trusted block."""
        model, core, nz = self.model, self.body_model.bm, self.Normalizer
        dev = pose.device
        T, D = pose.shape
        n_steps = len(t_list)
        net = ScoreNetCall(model, self.sde, bool(getattr(self, "continuous", True)), T, n_steps, dev)      # (the weights are packed once per loop)
        eng, lib = net.eng, _C.lib()
        F = int(frames_per_sequence) if frames_per_sequence else T
        n_seq = T // F
        if betas is None:
            betas = self.betas if self.betas.shape[0] == T else self.betas[:1]
        if betas.shape[0] > 1 and bool((betas == betas[:1]).all()):
            # one body shape for every frame (the module's default: motion_denoising.py:64 keeps zeros((batch_size, 10))): the rest
            # shape is formed once and shared -- the skinning kernels then read 126 KB from L2 instead of a [T, V, 3] copy from HBM
            # in every step (0.97 GB forward and again backward at 7680 frames); row b of the batched result carries the same bits
            betas = betas[:1]
        v_shaped, j_rest, batched = core.rest_shape(betas.contiguous(), None)
        v_shaped, j_rest = v_shaped.contiguous(), j_rest.contiguous()
        if batched and v_shaped.shape[0] == 1 and T > 1:
            batched = False                                        # [1, V, 3] / [1, J, 3] read as the shared [V, 3] / [J, 3]
        body = BodyTables(core, landmarks=True)
        body_fields = body.fields(T, dev)
        scratch = torch.empty(int(lib.dposer_motion_denoise_scratch_bytes(T, D, core.V, body.rows)), dtype=torch.uint8, device=dev)
        m, v = torch.zeros_like(pose), torch.zeros_like(pose)
        log = torch.zeros(n_steps, n_seq, 3, dtype=torch.float32, device=dev)
        rot6d = getattr(nz, "rot_rep", "axis") == "rot6d"          # the network sees 6 J coordinates; the optimised pose stays axis-angle
        if rot6d and eng.D != 2 * D:
            raise _C.DPoserHipError(f"rot_rep='rot6d': the score network takes {eng.D} inputs, the pose has {D} axis-angle parameters")
        obs = init_joints.detach().contiguous().float()
        conf_d = None if conf is None else conf.detach().to(dev).contiguous().float()
        rows_d = None if obs_rows is None else torch.tensor(list(obs_rows), dtype=torch.int32, device=dev)
        if conf_d is not None and tuple(conf_d.shape) != tuple(obs.shape[:2]):
            raise ValueError(f"joints_conf must be {list(obs.shape[:2])}, got {list(conf_d.shape)}")
        if rows_d is not None and (rows_d.numel() != obs.shape[1] or min(obs_rows) < 0 or max(obs_rows) >= core.J or len(set(obs_rows)) != len(obs_rows)):
            raise ValueError(f"obs_joints must be {obs.shape[1]} distinct tree joints in [0, {core.J}), got {list(obs_rows)}")
        mode, na, nb = normalizer_tables(nz, pose)
        nzs = None if noise is None else noise.detach().contiguous().float()
        if nzs is not None and tuple(nzs.shape) != (n_steps, T, eng.D):
            # the C loop indexes the noise as noise + k * T * D_net: [steps, T, 6 J] with rot_rep = 'rot6d', [steps, T, 3 J] otherwise
            raise _C.DPoserHipError(f"noise must be [n_steps, frames, network inputs] = {(n_steps, T, eng.D)}, got {tuple(nzs.shape)}")
        step0 = self._calls + 1
        self._calls += n_steps
        a = _C.MotionDenoiseArgs(
            **net.fields(), **body_fields, j_rest=_C.ptr(j_rest), v_shaped=_C.ptr(v_shaped), rest_batched=1 if batched else 0,
            frames=T, frames_per_sequence=F, pose=_C.ptr(pose),
            adam_m=_C.ptr(m), adam_v=_C.ptr(v), joints_obs=_C.ptr(obs), n_obs_joints=int(obs.shape[1]), norm_mode=mode, norm_a=_C.ptr(na),
            norm_b=_C.ptr(nb), n_steps=n_steps, weighted=0, t_host=float_array(t_list), w_temp_host=float_array(weights["temp"](1.0, it) for it in its),
            w_data_host=float_array(weights["data"](1.0, it) for it in its), w_prior_host=float_array(weights["dposer"](1.0, it) for it in its),
            lr=0.03, beta1=0.9, beta2=0.999, eps=1e-8, adam_step0=0, step0=int(step0) & 0xFFFFFFFF, seed=int(model._rng_seed + 31),
            noise=_C.ptr(nzs), scratch=_C.ptr(scratch), loss_log=_C.ptr(log), rot6d=1 if rot6d else 0,
            joints_conf=_C.ptr(conf_d), obs_rows=_C.ptr(rows_d))
        _C.check(lib.dposer_motion_denoise_optimize(C.byref(a), _C.stream_ptr()), "dposer_motion_denoise_optimize")
        self.adam_state = (m, v)                                   # torch.optim.Adam's exp_avg / exp_avg_sq after the last step (of the last call), [T, 63]
        return log

    def _quan_t(self, time_strategy, step, total_steps, sample_trun, sample_time):
        if time_strategy == "1":
            return int(torch.randint(self.sde.N, [1]))
        if time_strategy == "2":
            return int(sample_time)
        if time_strategy == "3":
            return int(self.sde.N - math.floor(float(np.float32(total_steps - step - 1) * np.float32(self.sde.N / (sample_trun * total_steps)))) - 2)
        raise NotImplementedError("unsupported time sampling strategy")

    def optimize_sequences(self, joints3d, gt_poses, time_strategy="3", sample_trun=2.0, sample_time=990, iterations=5, steps_per_iter=50,
                           noise=None, init_poses=None, joints_conf=None, obs_joints=None):
        """A BATCH of sequences advanced together by the one-call loop: joints3d [S, F, 22, 3], gt_poses / init_poses [S, F, 63],
        noise [steps, S * F, 63] or None.  Every sequence is the independent problem ``optimize`` solves (same schedule, same loss
        weights; temporal neighbours, data-term decision and loss means per sequence), but the S * F frames share every launch --
        one 60-frame sequence leaves most of an MI355X idle (GPU-bound small kernels), and under data parallelism
        each rank takes its shard of the sequences.  Returns the ``optimize`` metrics as [S, F] arrays and pose_body [S, F, 63].
        ``joints_conf`` [F, n_obs] or [S, F, n_obs] / ``obs_joints``: partial observations, as in ``optimize`` (joints3d is then
        [S, F, n_obs, 3])."""
        S, F = joints3d.shape[:2]
        conf, rows = _partial_observation(joints3d, joints_conf, obs_joints, getattr(getattr(self.body_model, "bm", None), "J", 22))
        partial = conf is not None or rows is not None
        names = ("init_MPJPE", "MPJPE", "MPVPE") + (("MPJPE_observed", "MPJPE_unobserved") if partial else ())
        if not self._fused_supported():
            # configurations outside the one-call loop (6D rotations, the VE SDE, a non-positional embedding): every sequence through
            # `optimize`'s step-by-step loop, one after the other -- same results layout, none of the batching
            if F != self.batch_size:
                raise ValueError(f"optimize_sequences: {F} frames per sequence, the module was built for batch_size = {self.batch_size}")
            res = [self.optimize(joints3d[i], gt_poses[i], time_strategy=time_strategy, sample_trun=sample_trun, sample_time=sample_time,
                                 iterations=iterations, steps_per_iter=steps_per_iter,
                                 noise=None if noise is None else noise[:, i * F:(i + 1) * F],
                                 init_poses=None if init_poses is None else init_poses[i], fused=False,
                                 **({"joints_conf": None if conf is None else conf[i], "obs_joints": rows} if partial else {})) for i in range(S)]
            out = {k: np.stack([np.asarray(r[k]) for r in res]) for k in names}
            out["pose_body"] = torch.stack([r["pose_body"] for r in res])
            return out
        bm = self.body_model
        flat = lambda x: x.reshape(S * F, *x.shape[2:])
        # (the body shapes the loop itself uses, _optimize_fused: one per frame of the batch if the module holds S * F of them)
        betas = self.betas if self.betas.shape[0] == S * F else self.betas[:1].expand(S * F, -1).contiguous()
        with torch.no_grad():
            gt = bm(betas=betas, pose_body=flat(gt_poses))
            if not partial:
                je = flat(joints3d) - gt.Jtr[:, :22]
                init_mpjpe = torch.mean(torch.sqrt(torch.sum(je * je, dim=2)), dim=1) * 100.0
        conf_flat = None if conf is None else flat(conf)
        timesteps = torch.linspace(self.sde.T, 1e-3, self.sde.N)
        total_steps = iterations * steps_per_iter
        # (every sequence starts from the module's random initial poses, as `optimize` does: frames must differ -- two identical
        #  neighbouring frames give the temporal term's sqrt a zero argument and a NaN gradient, in the reference too)
        start = self.poses[:F].repeat(S, 1) if init_poses is None else flat(init_poses)
        pose = start.detach().clone().contiguous().float()
        quan = [self._quan_t(time_strategy, step, total_steps, sample_trun, sample_time) for step in range(total_steps)]
        # (the C entry takes at most 65535 frames per call -- one grid row per frame in its skinning kernels; sequences are independent
        #  problems, so a larger batch goes through in groups of whole sequences, each group with its rows of the injected noise)
        per_call = max(1, 65535 // F)
        joints_flat, t_steps = flat(joints3d).detach(), [float(timesteps[q]) for q in quan]
        iters_of_step, weights, logs = [s // steps_per_iter for s in range(total_steps)], self.get_loss_weights(), []
        for s0 in range(0, S, per_call):
            fr = slice(s0 * F, min(S, s0 + per_call) * F)
            logs.append(self._optimize_fused(pose[fr], joints_flat[fr], t_steps, iters_of_step, weights,
                                             None if noise is None else (noise if per_call >= S else noise[:, fr].contiguous()),
                                             frames_per_sequence=F,
                                             betas=self.betas[fr] if (per_call < S and self.betas.shape[0] == S * F) else None,
                                             conf=None if conf_flat is None else conf_flat[fr], obs_rows=rows))
        self.loss_log = logs[0] if len(logs) == 1 else torch.cat(logs, dim=1)
        with torch.no_grad():
            final = pose.reshape(S, F, -1)
            smooth = torch.stack([gaussian_smoothing(final[i], window_size=3, sigma=2) for i in range(S)])
            smooth[:, [0, -1]] = final[:, [0, -1]]
            out = bm(betas=betas, pose_body=flat(smooth))
            je = out.Jtr[:, :22] - gt.Jtr[:, :22]
            ve = out.v - gt.v
            mpjpe = torch.mean(torch.sqrt(torch.sum(je * je, dim=2)), dim=1) * 100.0
            mpvpe = torch.mean(torch.sqrt(torch.sum(ve * ve, dim=2)), dim=1) * 100.0
            extra = _partial_metrics(joints_flat, conf_flat, rows, gt.Jtr, out.Jtr) if partial else {}
        r = lambda x: x.reshape(S, F).cpu().numpy()
        if partial:
            init_mpjpe = extra.pop("init_MPJPE")
        return dict({"init_MPJPE": r(init_mpjpe), "MPJPE": r(mpjpe), "MPVPE": r(mpvpe), "pose_body": final}, **{k: r(v) for k, v in extra.items()})

    @staticmethod
    def visualize(vertices, faces, out_path, render=False, prefix="out", save_mesh=False, faster=False, device=None):
        """motion_denoising.py:175-197: meshes as ``meshes/{prefix}_%04d.obj`` and / or renders as ``renders/{prefix}_%04d.png`` (front
        view over the white 512 x 384 canvas, every frame in one render call) or, with ``faster``, ``renders/{prefix}_%04d.jpg`` through
        ``faster_render``."""
        from ..body_model import visual
        os.makedirs(out_path, exist_ok=True)
        if save_mesh:
            v, f = vertices.detach().cpu().numpy(), np.asarray(faces.cpu() if torch.is_tensor(faces) else faces)
            os.makedirs(os.path.join(out_path, "meshes"), exist_ok=True)
            for i in range(len(v)):
                visual.save_obj(v[i], f, os.path.join(out_path, "meshes", "{}_{:04}.obj".format(prefix, i)))
        if render:
            target = os.path.join(out_path, "renders")
            os.makedirs(target, exist_ok=True)
            if faster:
                assert device is not None
                visual.faster_render(vertices, faces, target, prefix + "_{:04}.jpg", device)
            else:
                H, W = VIS_CANVAS
                dev = vertices.device if torch.is_tensor(vertices) and vertices.is_cuda else visual._dev()
                rgb, mask = visual._render_mesh_batch(vertices, faces, H, W, VIS_FOCAL, VIS_PRINCPT, ["front"] * len(vertices), dev)
                white = torch.full_like(rgb, 255)
                rgb = torch.where(mask[..., None], rgb, white).cpu().numpy()
                for i in range(len(rgb)):
                    visual.write_image(os.path.join(target, "{}_{:04}.png".format(prefix, i)), rgb[i])

    def optimize(self, joints3d, gt_poses=None, time_strategy="1", sample_trun=2.0, sample_time=990, iterations=5, steps_per_iter=50,
                 verbose=False, vis=False, noise=None, init_poses=None, fused=None, joints_conf=None, obs_joints=None):
        """motion_denoising.py:199-300.  Returns {'init_MPJPE', 'MPJPE', 'MPVPE'} in cm per frame.
        ``fused``: None = the one-call loop when the configuration supports it, False = step by step through autograd.
        ``vis``: also write the skeleton frames, ``gt_*`` / ``out_*`` renders, ``merges/`` and the motion video into ``self.out_path``
        (the video as ``motion.avi``, see utils.motion_video.write_video); the returned metrics do not depend on it.

        PARTIAL OBSERVATIONS (the rule is written out at dposer_motion_denoise_args, include/dposer_hip.h; both paths apply it):
        ``obs_joints``: a host list of distinct tree joints, one per column of ``joints3d`` [F, n_obs, 3] (None: column j is joint j);
        ``joints_conf`` [F, n_obs]: the confidence of every entry (None: 1).  An entry with a confidence that is not > 0 is not read (it may
        be NaN); the data term is the confidence-weighted mean distance over the others; a sequence without any keeps moving under the prior
        and the temporal term.  With either argument ``init_MPJPE[t]`` is the mean over frame t's live entries (NaN without one) and the
        result gains ``MPJPE_observed`` / ``MPJPE_unobserved``: the first 22 joints split by whether the frame observes them (NaN where
        the set is empty).  With neither, nothing changes."""
        bm = self.body_model
        if vis and self.out_path is None:
            raise ValueError("optimize(vis=True) needs the module's out_path")
        conf, rows = _partial_observation(joints3d, joints_conf, obs_joints, getattr(getattr(bm, "bm", None), "J", 22))
        partial = conf is not None or rows is not None
        if vis and partial:
            raise NotImplementedError("optimize(vis=True) does not plot partial observations (skeletons with NaN joints)")
        with torch.no_grad():
            gt = bm(betas=self.betas, pose_body=gt_poses)
            if vis:
                from ..body_model.visual import vis_skeletons
                vis_skeletons(joints3d.detach().cpu().numpy(), os.path.join(self.out_path, "renders"))
                print("skeleton figures saved")
                self.visualize(gt.v, gt.f, self.out_path, render=True, prefix="gt", device=self.device)
            if not partial:
                joint_error = joints3d - gt.Jtr[:, :22]
                init_mpjpe = torch.mean(torch.sqrt(torch.sum(joint_error * joint_error, dim=2)), dim=1) * 100.0
        init_joints = joints3d.detach()
        weights = self.get_loss_weights()
        timesteps = torch.linspace(self.sde.T, 1e-3, self.sde.N)
        total_steps = iterations * steps_per_iter
        use_fused = self._fused_supported() if fused is None else bool(fused)
        if use_fused:
            if not self._fused_supported():
                raise NotImplementedError("the one-call motion-denoising loop covers axis-angle / rot6d poses and sub-VP / VP SDEs")
            pose = (self.poses if init_poses is None else init_poses).detach().clone().contiguous().float()
            quan = [self._quan_t(time_strategy, step, total_steps, sample_trun, sample_time) for step in range(total_steps)]
            self.loss_log = self._optimize_fused(pose, init_joints, [float(timesteps[q]) for q in quan],
                                                 [s // steps_per_iter for s in range(total_steps)], weights, noise, conf=conf, obs_rows=rows)
        else:
            pose = (self.poses if init_poses is None else init_poses).clone().detach().requires_grad_(True)
            optimizer = torch.optim.Adam([pose], 0.03, betas=(0.9, 0.999))
            if partial:
                live = torch.ones(init_joints.shape[:2], dtype=torch.bool, device=init_joints.device) if conf is None else conf > 0
                cw = torch.where(live, torch.ones_like(init_joints[..., 0]) if conf is None else conf.to(init_joints.dtype), torch.zeros_like(init_joints[..., 0]))
                cols = list(range(init_joints.shape[1])) if rows is None else rows
            for it in range(iterations):
                for i in range(steps_per_iter):
                    step = it * steps_per_iter + i
                    optimizer.zero_grad()
                    poses_n = _normalize_with_grad(self.Normalizer, pose)
                    q = self._quan_t(time_strategy, step, total_steps, sample_trun, sample_time)
                    losses = {"dposer": self.DPoser_loss(poses_n, float(timesteps[q]), z=None if noise is None else noise[step])}
                    body = bm(betas=self.betas, pose_body=pose)                          # forward WITH gradient
                    temp = body.v[:-1] - body.v[1:]
                    losses["temp"] = torch.mean(torch.sqrt(torch.sum(temp * temp, dim=2)))
                    if partial:
                        losses["data"] = self._partial_data_term(body.Jtr[:, cols], init_joints, live, cw)
                    else:
                        data = body.Jtr[:, :22] - init_joints
                        # motion_denoising.py:262 keeps the data term only `if data_term > 0` ("for nans"): a host sync per step whose
                        # real job is the all-zero case (pose still equal to the observation: value 0, but sqrt'(0) = inf poisons the
                        # backward pass).  Same effect without the sync: distances are clamped away from 0 before the sqrt, so a zero
                        # residual contributes the value ~0 and a ZERO gradient, and a non-finite / non-positive term is dropped by value.
                        dist = torch.sqrt(torch.sum(data * data, dim=2).clamp_min(1e-36))
                        data_term = torch.mean(dist)
                        losses["data"] = torch.where(torch.isfinite(data_term) & (data_term > 0), data_term, torch.zeros_like(data_term))
                    tot = torch.stack([weights[k](v, it) for k, v in losses.items()]).sum()
                    tot.backward()
                    optimizer.step()
        with torch.no_grad():
            final = pose.detach()
            smooth = gaussian_smoothing(final, window_size=3, sigma=2)
            smooth[[0, -1]] = final[[0, -1]]
            out = bm(betas=self.betas, pose_body=smooth)
            if vis:
                from ..utils.motion_video import seq_to_video
                self.visualize(out.v, out.f, self.out_path, render=True, prefix="out", device=self.device)
                seq_to_video(os.path.join(self.out_path, "renders"), os.path.join(self.out_path, "merges"),
                             video_path=os.path.join(self.out_path, "motion.mp4"))
            je = out.Jtr[:, :22] - gt.Jtr[:, :22]
            ve = out.v - gt.v
            mpjpe = torch.mean(torch.sqrt(torch.sum(je * je, dim=2)), dim=1) * 100.0
            mpvpe = torch.mean(torch.sqrt(torch.sum(ve * ve, dim=2)), dim=1) * 100.0
            extra = _partial_metrics(init_joints, conf, rows, gt.Jtr, out.Jtr) if partial else {}
        if partial:
            init_mpjpe = extra.pop("init_MPJPE")
        return dict({"init_MPJPE": init_mpjpe.cpu().numpy(), "MPJPE": mpjpe.cpu().numpy(), "MPVPE": mpvpe.cpu().numpy(), "pose_body": final},
                    **{k: v.cpu().numpy() for k, v in extra.items()})

    @staticmethod
    def _partial_data_term(joints, obs, live, cw):
        """The data term of partial observations in torch, for the step-by-step path -- the rule of dposer_motion_denoise_args: joints
        [F, n_obs, 3] (the observed tree joints, with gradient), obs [F, n_obs, 3], live [F, n_obs] = confidence > 0, cw = the confidence
        where live and 0 elsewhere.  No host sync: the decision is a tensor.  What is not live, and every entry of a dropped term, is
        replaced by a finite residual before the sqrt, so its gradient is an exact 0 and not 0 x NaN."""
        with torch.no_grad():
            r = torch.where(live[..., None], joints - obs, torch.zeros_like(joints))
            W = cw.sum()
            value = (cw * torch.sqrt(torch.sum(r * r, dim=2).clamp_min(1e-36))).sum() / W      # (a NaN under a live entry stays NaN; 0 / 0 without live entries)
            keep = (W > 0) & torch.isfinite(value) & (value > 0)
        use = live & keep
        r = torch.where(use[..., None], joints - torch.where(use[..., None], obs, torch.zeros_like(obs)), torch.zeros_like(joints))
        s2 = torch.sum(r * r, dim=2)
        dist = torch.sqrt(s2.clamp_min(1e-36))
        w = torch.where(use, cw, torch.zeros_like(cw))
        return (w * dist).sum() / torch.where(keep, W, torch.ones_like(W))


def evaluate_motion_denoising(md, joints3d, gt_poses, *, sequences_per_call=32, num_replicas=None, rank=None, **optimize_kwargs):
    """The dataset loop of run/motion_denoising.py (its ``__main__`` walks the test sequences one at a time, one process) for a set
    of equal-length sequences, data parallel over SEQUENCES -- the frames of one sequence are coupled by the temporal term, so that
    is the only axis that shards: this rank's contiguous shard (``distributed.shard_bounds``, the reference's
    DistributedEvalSampler arithmetic), ``sequences_per_call`` sequences advanced together by ``optimize_sequences``, per-frame
    metrics kept as device-side sums, ONE all-reduce of (sum, count) pairs at the end (``distributed.reduce_metric_means``).
    ``joints3d`` [S, F, 22, 3] noisy observations, ``gt_poses`` [S, F, 63].  Returns ({'init_MPJPE', 'MPJPE', 'MPVPE'} means in cm over
    every frame of every rank, sequences evaluated here).
    ``joints_conf`` [F, n_obs] or [S, F, n_obs] / ``obs_joints``: partial observations as in ``MotionDenoise.optimize`` (joints3d is then
    [S, F, n_obs, 3]).  The means gain 'MPJPE_observed' and 'MPJPE_unobserved', and every metric is averaged over its non-NaN frames (a
    frame without a live entry has no init_MPJPE, a fully observed one no MPJPE_unobserved)."""
    from .. import distributed as ddp
    world = ddp.world_size() if num_replicas is None else num_replicas
    rk = ddp.rank() if rank is None else rank
    lo, hi = ddp.shard_bounds(joints3d.shape[0], world, rk)
    joints_conf, obs_joints = optimize_kwargs.pop("joints_conf", None), optimize_kwargs.pop("obs_joints", None)
    partial = joints_conf is not None or obs_joints is not None
    names = ("MPJPE", "MPVPE", "init_MPJPE") + (("MPJPE_observed", "MPJPE_unobserved") if partial else ())
    if partial:
        optimize_kwargs["obs_joints"] = obs_joints
    per_sequence = joints_conf is not None and len(joints_conf.shape) == 3
    results = []
    for s0 in range(lo, hi, sequences_per_call):
        s1 = min(s0 + sequences_per_call, hi)
        if partial:
            optimize_kwargs["joints_conf"] = joints_conf[s0:s1] if per_sequence else joints_conf
        res = md.optimize_sequences(joints3d[s0:s1], gt_poses[s0:s1], **optimize_kwargs)
        batch = {k: torch.as_tensor(res[k]).reshape(-1) for k in names}
        # (the NaN frames leave before the (sum, count) pairs are formed: a metric's mean is over the frames that have it)
        results.append({k: v[~torch.isnan(v)] for k, v in batch.items()} if partial else batch)
    return ddp.reduce_metric_means(results, device=joints3d.device, names=names), hi - lo

