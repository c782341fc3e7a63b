"""CPU restatement of the reference's task loops around the DPoser prior -- TEST INFRASTRUCTURE (see oracle/__init__.py).

* ``completion_optimize``      run/completion.py:167-207 (``DPoserComp.optimize``) with the loss of :131-149, the weights of
                               :151-155 and ``backward_step`` :157-165.
* ``motion_denoise_optimize``  run/motion_denoising.py:199-300 (``MotionDenoise.optimize``) with ``DPoser_loss`` :124-143, the
                               weights of :157-163, the ``if data_term > 0`` guard :261-263 and the final Gaussian smoothing
                               (lib/utils/misc.py:84-95).  Its defaults are the loop golden g15 pins; with ``dtype=torch.float64``
                               it is the arbiter of the one-call loop in every configuration that loop takes (normalisers, rot6d,
                               SDE kinds, embeddings, batches of sequences, per-frame betas), step by step and term by term
                               (tests/motion_denoise_cases.py, tests/test_motion_denoise_ref_cpu.py, tests/test_gpu_motion_denoise.py).

* ``smplify_optimize``         run/smplify.py:182-281 (``SMPLify.__call__``) with the losses of lib/body_model/fitting_losses.py:6-131,
                               the prior of run/smplify.py:93-115 and the stage weights of :145-149 -- float64 by default, the
                               arbiter of the one-call loop's outputs AND of its per-iteration loss log.

PINNED: ``tests/golden/g14_completion_loop.npz`` and ``g15_motion_denoise_loop.npz`` hold outputs of the reference's OWN loops
(``run.completion.DPoserComp.optimize`` / ``run.motion_denoising.MotionDenoise.optimize`` imported in the build container,
``tests/golden/gen_golden.py g14 g15``), and ``tests/test_oracle_golden.py`` checks these restatements against them.  The body
model handed to the reference's motion-denoising loop is ``oracle.fk_torch`` on the synthetic SMPL-X-shaped asset (smplx itself
is absent), so g15 pins the LOOP -- weights, time schedule, guard, optimiser, smoothing, metrics -- not the LBS arithmetic.
``g27_smplify.npz`` holds the reference's own ``SMPLify.__call__`` over the same body-model stand-in (every iteration's parameters, the
outputs, loss values and gradients at fixed inputs); ``tests/test_smplify_ref_cpu.py`` checks ``smplify_optimize`` against it.
"""
import math

import numpy as np
import torch

from . import fk_torch
from . import score_ref as R


def quan_t_strategy3(step: int, total_steps: int, N: int, sample_trun: float) -> int:
    """``N - floor(tensor(total - step - 1) * (N / (trun * total))) - 2`` (completion.py:189-190, motion_denoising.py:245): an int64
    tensor times a python float is evaluated in fp32."""
    return int(N - math.floor(float(np.float32(total_steps - step - 1) * np.float32(N / (sample_trun * total_steps)))) - 2)


def completion_optimize(p, sde, observation, mask, noise, *, iterations=2, steps_per_iter=100, lr=0.1, sample_trun=5.0):
    """run/completion.py:167-207, time strategy '3'.  ``noise[step]`` is the z of completion.py:133.
    The reference passes ``quan_t`` positionally into ``weighted`` (:196), i.e. weighted = bool(quan_t)."""
    obs = torch.as_tensor(observation, dtype=torch.float32)
    msk = torch.as_tensor(mask, dtype=torch.float32)
    x = obs.clone().requires_grad_(True)
    opt = torch.optim.Adam([x], lr, betas=(0.9, 0.999))
    ts = torch.linspace(1.0, 1e-3, sde.N)
    total = iterations * steps_per_iter
    for it in range(iterations):
        for i in range(steps_per_iter):
            step = it * steps_per_iter + i
            opt.zero_grad()
            q = quan_t_strategy3(step, total, sde.N, sample_trun)
            t = torch.ones(x.shape[0]) * ts[q]
            _, g = R.dposer_prior_loss(p, sde, x.detach(), t, torch.as_tensor(noise[step]), weighted=bool(q), reduction="mean")
            ld = torch.nn.functional.mse_loss(x * msk, obs * msk)                  # data_loss, :197
            (100 * ld / (1 + it)).backward()                                       # weights :151-155
            x.grad += 0.1 * (it + 1) * g
            opt.step()
    return (obs * msk + x.detach() * (1.0 - msk)).numpy()


def gaussian_smoothing(x, window_size=3, sigma=2.0):
    """lib/utils/misc.py:84-95: depth-wise 1-D Gaussian filter along the frame axis, zero padded."""
    k = torch.arange(window_size, dtype=x.dtype) - window_size // 2
    w = torch.exp(-0.5 * (k / sigma) ** 2)
    w = w / w.sum()
    xt = x.t()[None]                                                               # [1, D, T]
    pad = window_size // 2
    out = torch.nn.functional.conv1d(torch.nn.functional.pad(xt, (pad, pad)), w.view(1, 1, -1).repeat(x.shape[1], 1, 1), groups=x.shape[1])
    return out[0].t()


# the faults ``motion_denoise_optimize(fault=...)`` can seed into itself: tests/test_motion_denoise_ref_cpu.py shows that each one leaves
# the comparison band of tests/test_gpu_motion_denoise.py, i.e. that a kernel with that defect could not pass
MOTION_DENOISE_FAULTS = ("temporal_crosses_sequences", "temporal_mean_over_T", "data_guard_ignored", "data_mean_over_frames", "min_max_without_2",
                         "prior_grad_not_divided_by_std", "rot6d_grad_not_through_rodrigues", "prior_weight_of_previous_iteration",
                         "noise_row_shifted", "weighted_on")


def motion_denoise_optimize(p, sde, asset, mean, std, joints3d, gt_poses, init_poses, noise, *, iterations=5, steps_per_iter=50,
                            sample_trun=2.0, dposer_weight=1.0, body_dtype=torch.float64, dtype=None, norm_mode="zscore", rot6d=False,
                            embedding_type="positional", weighted=False, time_strategy="3", sample_time=990, betas=None, n_obs_joints=22,
                            frames_per_sequence=None, fault=None, details=False):
    """run/motion_denoising.py:199-300.  With the defaults: time strategy '3', z-score normaliser, returns (final pose_body before
    smoothing, {'init_MPJPE', 'MPJPE', 'MPVPE'}); the body model is fk_torch (float64; ``body_dtype=torch.float32`` = the precision smplx
    runs in inside the reference), poses are an fp32 leaf and the network runs in fp32 like in the reference -- the loop golden g15 pins.

    ``dtype``: None = that mixed loop; torch.float64 / torch.float32 = EVERYTHING in that precision -- network, body model, pose leaf,
    Adam: float64 is the arbiter of the one-call loop, float32 sizes the reference's own rounding.
    ``norm_mode``: None / 'none', 'zscore' (``mean``, ``std`` = the statistics) or 'minmax' (``mean``, ``std`` = min, max);  ``rot6d``: the
    network sees the 6 J coordinates of ``smplify_normalize`` and its gradient returns through autograd of that conversion (noise and
    statistics are 6 J wide);  the SDE kind is ``sde`` (R.SubVP / R.VP / R.VE, ``discrete=True`` for the discrete score functions);
    ``embedding_type``: 'positional' or 'fourier';  ``weighted``: DPoser_loss's flag (:124, False in the reference);  ``time_strategy``
    '2' (the fixed ``sample_time``) or '3';  ``betas`` [frames, 10] or [1, 10]: body shapes (None: zeros);  ``n_obs_joints``: the first
    joints the data term (and init_MPJPE) reads.
    ``frames_per_sequence`` F: the frames are S = frames / F sequences of F consecutive frames, S independent problems: every loss
    term, its mean, the ``data_term > 0`` decision and the prior (``sum_over_batch`` with batch_size = F, what one sequence alone gets) are
    formed on the sequence's slice; Adam is element-wise, so this IS S runs of the reference loop on slices of pose, observation and noise.
    ``fault``: one of MOTION_DENOISE_FAULTS, seeded on purpose.

    ``details=True`` returns a dict instead: pose [T, D] (final, before smoothing), pose_steps [steps, T, D] (after every step), grad_steps
    [steps, T, D] (the total gradient handed to Adam), adam_m / adam_v (after the last step), log [steps, S, 3] (temp, data, prior:
    unweighted, data = 0 where the guard dropped it, prior = the sequence's own term), data_kept [steps, S] and the three metrics [T]
    (after the Gaussian smoothing, per sequence)."""
    assert fault is None or fault in MOTION_DENOISE_FAULTS, fault
    legacy = dtype is None
    if legacy:
        dtype = torch.float32
    else:
        body_dtype = dtype
    T = init_poses.shape[0]
    F = int(frames_per_sequence) if frames_per_sequence else T
    S = T // F
    assert S * F == T and F >= 2
    seqs = [slice(s * F, (s + 1) * F) for s in range(S)]
    if norm_mode is None:
        norm_mode = "none"
    if fault == "weighted_on":
        weighted = True
    pd = {k: v.to(dtype) if v.is_floating_point() else v for k, v in p.items()}
    fw = {} if embedding_type == "positional" else {"embedding_type": embedding_type}
    mean = None if norm_mode == "none" else torch.as_tensor(mean, dtype=dtype)
    std = None if norm_mode == "none" else torch.as_tensor(std, dtype=dtype)
    joints = torch.as_tensor(joints3d, dtype=body_dtype)
    asset = {k: torch.as_tensor(v, dtype=body_dtype) if isinstance(v, np.ndarray) and v.dtype.kind == "f" else v for k, v in asset.items()}
    shape = None if betas is None else torch.as_tensor(betas, dtype=body_dtype).expand(T, -1)
    bm = lambda pose: fk_torch.smplx_forward(asset, pose.to(body_dtype), betas=shape, dtype=body_dtype)
    with torch.no_grad():
        v_gt, j_gt = bm(torch.as_tensor(gt_poses, dtype=dtype))
    je = joints - j_gt[:, :n_obs_joints]
    init_mpjpe = torch.mean(torch.sqrt(torch.sum(je * je, dim=2)), dim=1) * 100.0
    pose = torch.as_tensor(init_poses, dtype=dtype).clone().requires_grad_(True)
    opt = torch.optim.Adam([pose], 0.03, betas=(0.9, 0.999))
    ts = torch.linspace(1.0, 1e-3, sde.N)
    total = iterations * steps_per_iter
    z_all = torch.as_tensor(noise, dtype=dtype)
    mmf = 1.0 if fault == "min_max_without_2" else 2.0
    log = torch.zeros(total, S, 3, dtype=body_dtype)
    kept = np.zeros((total, S), dtype=bool)
    pose_steps, grad_steps = [], []
    for it in range(iterations):
        for i in range(steps_per_iter):
            step = it * steps_per_iter + i
            opt.zero_grad()
            q = int(sample_time) if time_strategy == "2" else quan_t_strategy3(step, total, sde.N, sample_trun)
            if not legacy:
                _smplify_check_label(sde, float(ts[q]))
            vec_t = torch.full((F,), float(ts[q]), dtype=dtype)
            z = z_all[min(step + 1, total - 1) if fault == "noise_row_shifted" else step]
            # offline_normalize(from_axis=True): z-score / min-max / none, after the 6-D conversion under rot6d
            x_n = smplify_normalize(pose, rot6d, norm_mode, mean, std, linear_rot6d_grad=fault == "rot6d_grad_not_through_rodrigues",
                                    min_max_factor=mmf)
            x0 = x_n.detach()
            # DPoser_loss(x_0, vec_t, quan_t, weighted=False) (:124, called :250): unweighted here -- unlike completion.py:196,
            # whose loss() has no quan_t parameter, so quan_t lands in `weighted` there
            gprior = torch.zeros_like(x0)
            for s, sl in enumerate(seqs):
                l_prior, gprior[sl] = R.dposer_prior_loss(pd, sde, x0[sl], vec_t, z[sl], weighted=weighted, reduction="sum_over_batch",
                                                          batch_size=F, **fw)
                log[step, s, 2] = l_prior
            v, j = bm(pose)
            itw = max(it - 1, 0) if fault == "prior_weight_of_previous_iteration" else it
            w_prior = 0.1 * (1 + itw) * dposer_weight                              # weights :157-163
            tots = []
            for s, sl in enumerate(seqs):
                if fault == "temporal_crosses_sequences" and s + 1 < S:
                    vs = v[sl.start:sl.stop + 1]
                    temp = vs[:-1] - vs[1:]
                    l_temp = torch.sum(torch.sqrt(torch.sum(temp * temp, dim=2))) / ((F - 1) * v.shape[1])
                else:
                    temp = v[sl][:-1] - v[sl][1:]
                    l_temp = torch.mean(torch.sqrt(torch.sum(temp * temp, dim=2)))
                    if fault == "temporal_mean_over_T":
                        l_temp = l_temp * (F - 1) / F
                data = j[sl, :n_obs_joints] - joints[sl]
                l_data = torch.mean(torch.sqrt(torch.sum(data * data, dim=2)))
                if fault == "data_mean_over_frames":
                    l_data = l_data * n_obs_joints
                tot = 10.0 * l_temp * (1 + it)
                keep = bool(l_data > 0) or fault == "data_guard_ignored"
                if keep:                                                           # :261-263
                    tot = tot + 100.0 * l_data / (1 + it * it)
                kept[step, s] = keep
                log[step, s, 0], log[step, s, 1] = l_temp.detach(), l_data.detach() if keep else 0.0
                tots.append(tot)
            tot = tots[0] if S == 1 else torch.stack(tots).sum()
            if rot6d:
                # x0_hat is detached (:102-104), so the prior reaches the pose through its analytic gradient and the conversion's autograd
                x_g = x_n if fault != "prior_grad_not_divided_by_std" else smplify_normalize(pose, True, "none", None, None)
                tot = tot + w_prior * (gprior.to(body_dtype) * x_g.to(body_dtype)).sum()
            tot.backward()
            if not rot6d:
                if norm_mode == "none" or fault == "prior_grad_not_divided_by_std":
                    gp = gprior
                elif norm_mode == "zscore":
                    gp = gprior / std
                else:
                    gp = mmf * gprior / (std - mean)
                pose.grad += w_prior * gp
            grad_steps.append(pose.grad.detach().clone())
            opt.step()
            pose_steps.append(pose.detach().clone())
    final = pose.detach()
    smooth = final.clone()
    for sl in seqs:
        smooth[sl] = gaussian_smoothing(final[sl], 3, 2.0)
        smooth[[sl.start, sl.stop - 1]] = final[[sl.start, sl.stop - 1]]
    with torch.no_grad():
        v, j = bm(smooth)
    je = j[:, :22] - j_gt[:, :22]
    ve = v - v_gt
    res = {"init_MPJPE": init_mpjpe.numpy(), "MPJPE": (torch.mean(torch.sqrt(torch.sum(je * je, dim=2)), dim=1) * 100.0).numpy(),
           "MPVPE": (torch.mean(torch.sqrt(torch.sum(ve * ve, dim=2)), dim=1) * 100.0).numpy()}
    if not details:
        return final.numpy(), res
    state = opt.state[pose]
    return dict(res, pose=final.numpy(), pose_steps=torch.stack(pose_steps).numpy(), grad_steps=torch.stack(grad_steps).numpy(),
                adam_m=state["exp_avg"].numpy(), adam_v=state["exp_avg_sq"].numpy(), log=log.numpy(), data_kept=kept)


# --------------------------------------------------------------------------------------------
# run/smplify.py + lib/body_model/fitting_losses.py
# --------------------------------------------------------------------------------------------
SMPLIFY_STAGE_WEIGHTS = {"pose_prior_weight": [50, 20, 10, 5, 2], "shape_prior_weight": [50, 20, 10, 5, 2],
                         "angle_prior_weight": [150, 50, 30, 15, 5]}                # smplify.py:147-149

# the faults ``smplify_optimize(fault=...)`` can seed into itself: tests/test_smplify_ref_cpu.py shows that each one leaves the
# comparison band, i.e. that a kernel with that defect could not pass
SMPLIFY_FAULTS = ("gt_fallback_ignored", "ign_joint_kept", "gmof_plain_square", "min_max_without_2", "angle_sign_55", "shape_grad_halved",
                  "prior_grad_0.9", "rot6d_grad_not_through_rodrigues", "noise_row_shifted")


def smplify_asset_subset(asset, joint_map):
    """The asset restricted to the vertices some mapped joint reads: the support of the joint regressor and the vertices of the mapped
    extra joints (no landmark rows).  Dropping a vertex that no output depends on changes no joint -- it only spares the loop the
    other 85 % of the mesh; tests/test_smplify_ref_cpu.py holds the mapped joints of both assets together."""
    nj = asset["J_regressor"].shape[0]
    ids = np.asarray(asset["extra_joint_vertex_ids"]).astype(np.int64)
    jm = np.asarray(joint_map).astype(np.int64)
    assert jm.max() < nj + len(ids), "landmark rows need whole faces"
    keep = np.union1d(np.nonzero((np.asarray(asset["J_regressor"]) != 0).any(axis=0))[0], ids)
    slot = -np.ones(asset["v_template"].shape[0], np.int64)
    slot[keep] = np.arange(len(keep))
    pdirs = np.asarray(asset["posedirs"])
    out = dict(asset)
    out.update(v_template=asset["v_template"][keep], shapedirs=asset["shapedirs"][keep], weights=asset["weights"][keep],
               J_regressor=asset["J_regressor"][:, keep], posedirs=pdirs.reshape(pdirs.shape[0], -1, 3)[:, keep].reshape(pdirs.shape[0], -1),
               extra_joint_vertex_ids=slot[ids], faces=np.zeros((0, 3), np.int64), lmk_faces_idx=np.zeros((0,), np.int64),
               lmk_bary_coords=np.zeros((0, 3), np.float32))
    return out


def smplify_project(joints, focal_length, camera_center):
    """fitting_losses.py:6-38 with rotation = I (:69,:114; the translation argument is never read): u = f x / z + c_x, v = f y / z + c_y."""
    f = torch.as_tensor(focal_length, dtype=joints.dtype).reshape(-1, 1)
    xy = joints[:, :, :2] / joints[:, :, 2:3]
    return f[:, :, None] * xy + camera_center[:, None, :]


def smplify_camera_terms(joints, cam_t, cam_t_est, camera_center, joints_2d, conf, focal_length, op_joints, gt_joints, depth_weight=100.0,
                         gt_fallback=True):
    """camera_fitting_loss, fitting_losses.py:106-136, per image: (reprojection [B], depth term [B]); the loss is the sum of both over
    the batch.  The OP hips / shoulders if all four OP confidences are > 0, else the four GT joints (:129-130)."""
    proj = smplify_project(joints, focal_length, camera_center)
    e_op = ((joints_2d[:, op_joints] - proj[:, op_joints]) ** 2).sum(dim=(1, 2))
    e_gt = ((joints_2d[:, gt_joints] - proj[:, gt_joints]) ** 2).sum(dim=(1, 2))
    valid = conf[:, op_joints].min(dim=-1)[0] > 0
    if not gt_fallback:
        valid = torch.ones_like(valid)
    return torch.where(valid, e_op, e_gt), depth_weight ** 2 * (cam_t[:, 2] - cam_t_est[:, 2]) ** 2


def smplify_gmof(x, sigma):
    """fitting_losses.py:41-47."""
    return (sigma ** 2 * x ** 2) / (sigma ** 2 + x ** 2)


def smplify_body_terms(body_pose, betas, joints, camera_center, joints_2d, conf, focal_length, sigma=100.0, shape_prior_weight=5.0,
                       angle_prior_weight=15.2, angle_signs=(1.0, -1.0, -1.0, -1.0), plain_square=False):
    """body_fitting_loss, fitting_losses.py:59-90, without the pose prior: (conf^2 (gmof(u - x) + gmof(v - y)) [B, K], w_angle^2 angle
    prior [B], w_shape^2 |betas|^2 [B]) -- each weighted as it enters the loss."""
    d = smplify_project(joints, focal_length, camera_center) - joints_2d
    rob = d ** 2 if plain_square else smplify_gmof(d, sigma)
    reproj = conf ** 2 * rob.sum(dim=-1)                                               # :74-75
    sg = torch.tensor(angle_signs, dtype=body_pose.dtype)
    angle = angle_prior_weight ** 2 * (torch.exp(body_pose[:, [52, 55, 9, 12]] * sg) ** 2).sum(dim=-1)      # :50-56, :84
    shape = shape_prior_weight ** 2 * (betas ** 2).sum(dim=-1)                        # :87
    return reproj, angle, shape


def _smplify_check_label(sde, t):
    """The index of the network's sigma table (model.py:159) and of the discrete VP std (utils.py:160) is ``(t * scale).long()`` of an fp32
    product in the reference; the float64 loop must land on the same integer, else it arbitrates another network input."""
    if sde.name == "VESDE":
        return
    scale = (sde.N - 1) if getattr(sde, "discrete", False) else 999
    if math.floor(float(np.float32(t) * np.float32(scale))) != math.floor(float(np.float32(t)) * scale):
        raise ValueError(f"time {t!r}: its label {scale} t truncates differently in fp32 and fp64; choose another schedule")


def smplify_normalize(body_pose, rot6d, norm_mode, norm_a, norm_b, *, linear_rot6d_grad=False, min_max_factor=2.0):
    """Posenormalizer.offline_normalize(from_axis=True), lib/dataset/AMASS.py:126-137 behind run/smplify.py:110: under rot6d the first two
    columns, row-major, of each joint's rotation matrix (lib/utils/transforms.py:238-261); then none / z-score / min-max."""
    x = body_pose
    if rot6d:
        rv = body_pose.reshape(-1, 3)
        six = fk_torch.batch_rodrigues(rv)[:, :, :2].reshape(body_pose.shape[0], -1)
        if linear_rot6d_grad:      # fault: the value of R(q), the gradient of I + [q]_x
            z, (rx, ry, rz) = torch.zeros_like(rv[:, 0]), rv.unbind(dim=1)
            lin = torch.stack([z + 1, -rz, rz, z + 1, -ry, rx], dim=1).reshape(body_pose.shape[0], -1)
            six = six.detach() + lin - lin.detach()
        x = six
    a = None if norm_a is None else torch.as_tensor(norm_a, dtype=x.dtype).reshape(1, -1)
    b = None if norm_b is None else torch.as_tensor(norm_b, dtype=x.dtype).reshape(1, -1)
    if norm_mode in (None, "none"):
        return x
    if norm_mode == "zscore":
        return (x - a) / b
    if norm_mode == "minmax":
        return min_max_factor * (x - a) / (b - a) - 1
    raise ValueError(norm_mode)


def smplify_optimize(p, sde, asset, joint_map, init_pose, init_betas, init_cam_t, camera_center, keypoints_2d, t_list, noise, *,
                     op_joints, gt_joints, ign_joints, focal_length=5000.0, num_iters=100, stage_weights=None, rot6d=False,
                     norm_mode="zscore", norm_a=None, norm_b=None, sigma=100.0, depth_weight=100.0, lr=1e-2, dtype=torch.float64,
                     fault=None):
    """run/smplify.py:182-281 with the prior noise injected (``noise[k]`` is the z of :96 at body iteration k) and the times given
    (``t_list[k]`` = ``pose_prior.timesteps[quan_t]``, :112,:250).  Everything -- body model, losses, prior network, Adam -- runs in
    ``dtype``: float64 is the arbiter, float32 sizes the reference's own rounding.

    ``joint_map`` [K]: rows of the body model's joint output (lib/body_model/smpl.py:55-57,70); ``op_joints`` / ``gt_joints`` /
    ``ign_joints``: keypoint indices of fitting_losses.py:118-121 and smplify.py:135-136.  ``norm_mode``: None, 'zscore' (a = mean,
    b = std) or 'minmax' (a = min, b = max).  ``fault``: one of SMPLIFY_FAULTS, seeded on purpose.

    Returns a dict: pose [B, 66], betas, cam_t, reprojection [B, K], conf [B, K] (ignored joints zeroed), it_orient / it_body_pose /
    it_betas / it_transl (the parameters at every body-model call: each iteration's start, then the finals), log
    [num_iters (1 + n_stages), B, 4] in the layout of include/dposer_hip.h (camera rows: camera loss, 0, 0, depth term; body rows:
    reprojection, angle, shape, prior -- weighted as they enter the loss, the prior being the whole batch's sum / batch_size) and
    prior_terms [n_stages num_iters, B]: each image's share of that prior entry."""
    assert fault is None or fault in SMPLIFY_FAULTS, fault
    sw = SMPLIFY_STAGE_WEIGHTS if stage_weights is None else stage_weights
    stages = [dict(zip(sw.keys(), vals)) for vals in zip(*sw.values())]               # smplify.py:239
    T = lambda a: torch.as_tensor(np.asarray(a), dtype=dtype).clone()
    pd = {k: v.to(dtype) if v.is_floating_point() else v for k, v in p.items()}
    init_pose, init_cam_t, center, kp = T(init_pose), T(init_cam_t), T(camera_center), T(keypoints_2d)
    B = init_pose.shape[0]
    focal = focal_length if np.ndim(focal_length) == 0 else T(focal_length)
    joint_map = torch.as_tensor(np.asarray(joint_map)).long()
    op_joints, gt_joints, ign_joints = list(op_joints), list(gt_joints), list(ign_joints)
    joints_2d, conf = kp[:, :, :2], kp[:, :, 2].clone()
    body_pose, orient = init_pose[:, 3:].clone(), init_pose[:, :3].clone()            # :194-196
    betas, cam_t = T(init_betas), init_cam_t.clone()
    z_all = T(noise)
    n_body = len(stages) * num_iters
    assert len(t_list) == n_body and tuple(z_all.shape[:2]) == (n_body, B)
    log = torch.zeros(num_iters + n_body, B, 4, dtype=dtype)
    prior_terms = torch.zeros(n_body, B, dtype=dtype)
    its = []
    # (converted once: smplx_forward's own as_tensor is then a no-op for the big blend-shape tables)
    asset = {k: torch.as_tensor(v, dtype=dtype) if isinstance(v, np.ndarray) and v.dtype.kind == "f" else v for k, v in asset.items()}

    def joints_of():
        its.append([x.detach().clone() for x in (orient, body_pose, betas, cam_t)])
        _, j = fk_torch.smplx_forward(asset, body_pose, betas=betas, global_orient=orient, transl=cam_t, dtype=dtype)
        return j[:, joint_map]

    # ---- camera stage, :198-221
    orient.requires_grad_(True)
    cam_t.requires_grad_(True)
    opt = torch.optim.Adam([orient, cam_t], lr=lr, betas=(0.9, 0.999))
    for k in range(num_iters):
        rep, depth = smplify_camera_terms(joints_of(), cam_t, init_cam_t, center, joints_2d, conf, focal, op_joints, gt_joints, depth_weight,
                                          gt_fallback=fault != "gt_fallback_ignored")
        log[k, :, 0], log[k, :, 3] = (rep + depth).detach(), depth.detach()
        opt.zero_grad()
        (rep + depth).sum().backward()                                                 # :135-136
        opt.step()
    cam_t = cam_t.detach()                                                             # :224
    conf[:, ign_joints[1:] if fault == "ign_joint_kept" else ign_joints] = 0.0          # :235
    # ---- body stage, :226-260
    body_pose.requires_grad_(True)
    betas.requires_grad_(True)
    opt = torch.optim.Adam([body_pose, betas, orient], lr=lr, betas=(0.9, 0.999))
    k = 0
    for w in stages:
        for _ in range(num_iters):
            _smplify_check_label(sde, t_list[k])
            rep, ang, shp = smplify_body_terms(body_pose, betas, joints_of(), center, joints_2d, conf, focal, sigma, w["shape_prior_weight"],
                                               w["angle_prior_weight"], angle_signs=(1.0, 1.0 if fault == "angle_sign_55" else -1.0, -1.0, -1.0),
                                               plain_square=fault == "gmof_plain_square")
            x_n = smplify_normalize(body_pose[:, :63], rot6d, norm_mode, norm_a, norm_b,
                                    linear_rot6d_grad=fault == "rot6d_grad_not_through_rodrigues",
                                    min_max_factor=1.0 if fault == "min_max_without_2" else 2.0)
            z = z_all[min(k + 1, n_body - 1) if fault == "noise_row_shifted" else k]
            vec_t = torch.full((B,), float(t_list[k]), dtype=dtype)
            # DPoser.DPoser_loss, smplify.py:93-107: x0_hat is detached (:73), so the prior reaches the pose through its analytic gradient
            prior, g = R.dposer_prior_loss(pd, sde, x_n.detach(), vec_t, z, weighted=True, reduction="sum_over_batch", batch_size=B)
            for b in range(B):
                prior_terms[k, b] = w["pose_prior_weight"] ** 2 * R.dposer_prior_loss(pd, sde, x_n[b:b + 1].detach(), vec_t[b:b + 1], z[b:b + 1],
                                                                                     weighted=True, reduction="sum_over_batch", batch_size=B)[0]
            if fault == "prior_grad_0.9":
                g = 0.9 * g
            if fault == "shape_grad_halved":
                shp_g = 0.5 * shp + 0.5 * shp.detach()
            else:
                shp_g = shp
            row = num_iters + k
            log[row, :, 0], log[row, :, 1], log[row, :, 2] = rep.sum(dim=-1).detach(), ang.detach(), shp.detach()
            log[row, :, 3] = w["pose_prior_weight"] ** 2 * prior.detach()
            # fitting_losses.py:90,103: the mean over the batch of (reprojection + prior + angle + shape); the prior is one scalar (:79)
            total = (rep.sum(dim=-1) + ang + shp_g).mean() + w["pose_prior_weight"] ** 2 * (g.detach() * x_n).sum()
            opt.zero_grad()
            total.backward()
            opt.step()
            k += 1
    # ---- final reprojection, :262-276
    with torch.no_grad():
        rep, _, _ = smplify_body_terms(body_pose, betas, joints_of(), center, joints_2d, conf, focal, sigma,
                                       plain_square=fault == "gmof_plain_square")
    stack = lambda i: torch.stack([c[i] for c in its]).numpy()
    return {"pose": torch.cat([orient, body_pose], dim=-1).detach().numpy(), "betas": betas.detach().numpy(), "cam_t": cam_t.numpy(),
            "reprojection": rep.numpy(), "conf": conf.numpy(), "it_orient": stack(0), "it_body_pose": stack(1), "it_betas": stack(2),
            "it_transl": stack(3), "log": log.numpy(), "prior_terms": prior_terms.numpy()}
