"""SMPLify: fitting SMPL-X to 2D keypoints under the DPoser prior -- counterpart of ``SMPLify`` in the reference's run/smplify.py:118-281
(the human-mesh-recovery application; losses in body_model/fitting_losses.py).

B independent images are fitted at once: a camera stage (Adam over global orientation and camera translation), then five body stages (a
fresh Adam over body pose, betas and global orientation) with the loss weights of smplify.py:145-149.

``fused=True`` (default) runs every iteration of both stages as ONE C call, ``dposer_smplify_optimize`` (csrc/smplify.hip): the body model
is a sub-mesh of just the vertices the 49-joint map reads, the loss gradients and the Adam updates are kernels, nothing returns to the host
in between.  ``fused=False`` is the step-by-step path -- the repository's SMPLX module, autograd and torch.optim.Adam -- and serves every
configuration the one-call loop does not cover (``SMPLify.fused_supported``).
"""
import ctypes as C
import math

import numpy as np
import torch

from .. import _C
from ..algorithms.advanced import sde_lib
from ..body_model import constants
from ..body_model.fitting_losses import body_fitting_loss, camera_fitting_loss
from ._fused import BodyTables, ScoreNetCall, float_array, normalizer_tables

_MAX_PER_CALL = 65535        # dposer_smplify_optimize: one grid row per pose in the skinning kernels


def _sub_mesh(smpl):
    """The body model the one-call loop runs: a core over only the vertices the extra joints of ``smpl.joint_map`` read.  The map's
    rows are derived from the map itself: tree joints [0, J) are the kinematic chain's; rows [J, J + n_extra) are vertex-selected extra
    joints; landmark rows would need whole faces and are not supported (returns None).  The rest joints come from the FULL asset's
    j_template / jdirs (dposer_shape_blend_forward takes V and J independently).  Returns (core, joint map onto the sub core's rows)."""
    from ..body_model.body_model import _SMPLCore
    core = smpl.bm
    dev = core.v_template.device
    cache = getattr(smpl, "_smplify_sub", None)
    if cache is not None and cache[0] == dev:
        return cache[1], cache[2]
    J, n_extra = core.J, core.n_extra
    jmap = smpl.joint_map.cpu().numpy().astype(np.int64)
    if (jmap >= J + n_extra).any():
        return None
    extra_rows = sorted({int(r) for r in jmap if r >= J})
    full_ids = core.extra_vertex_ids.cpu().numpy().astype(np.int64)
    verts = sorted({int(full_ids[r - J]) for r in extra_rows})
    vslot = {v: i for i, v in enumerate(verts)}
    nv = max(len(verts), 1)
    if not verts:
        verts = [0]
    cpu = lambda t: t.detach().cpu().numpy()
    vi = np.asarray(verts, dtype=np.int64)
    posedirs = cpu(core.posedirs).reshape(core.posedirs.shape[0], -1, 3)[:, vi].reshape(core.posedirs.shape[0], -1)
    asset = {"v_template": cpu(core.v_template)[vi], "shapedirs": cpu(core.shapedirs)[vi], "posedirs": posedirs,
             "J_regressor": np.zeros((J, nv), np.float32), "weights": cpu(core.lbs_weights)[vi], "parents": core._parents_np,
             "faces": np.zeros((0, 3), np.int64), "lmk_faces_idx": np.zeros((0,), np.int64), "lmk_bary_coords": np.zeros((0, 3), np.float32),
             "extra_joint_vertex_ids": np.asarray([vslot[int(full_ids[r - J])] for r in extra_rows], dtype=np.int32)}
    sub = _SMPLCore(asset, num_betas=core.num_betas, num_expression_coeffs=core.num_expression_coeffs, model_type=core.model_type)
    sub.j_template = core.j_template.detach().cpu().clone()
    sub.jdirs = core.jdirs.detach().cpu().clone()
    sub = sub.to(dev)
    row_of = {r: r for r in range(J)}
    row_of.update({r: J + e for e, r in enumerate(extra_rows)})
    sub_map = torch.tensor([row_of[int(r)] for r in jmap], dtype=torch.int32)
    smpl._smplify_sub = (dev, sub, sub_map)
    return sub, sub_map


class SMPLify:
    """run/smplify.py:118-281.  ``pose_prior``: a ``prior.DPoser`` to use instead of building one from ``args`` (e.g.
    ``DPoser(model=..., normalizer=...)`` over an in-memory network).  ``__call__`` returns (pose [B, 66], betas, camera_translation,
    reprojection_loss [B, 49]) like the reference; ``fused`` / ``noise`` [n_stages * num_iters, B, network inputs] / ``seed`` are this
    repository's keywords.

    ``loss_log`` (after a fused call): [num_iters * (1 + stages), B, 4], every iteration's loss terms per image as they enter the loss --
    camera rows (camera loss, 0, 0, depth term), body rows (reprojection, angle prior, shape prior, pose prior).  The pose prior is one
    scalar per C call: each image's row carries w_pose^2 * (sum over the images of ITS GROUP) / B.  One group (any B up to 65535) logs
    the loss's own sum / batch_size term in every row; with more groups the groups' values add up to that term."""

    def __init__(self, body_model, step_size=1e-2, batch_size=32, num_iters=100, focal_length=5000, args=None, pose_prior=None):
        from ..body_model.smpl import SMPLX
        from ..prior import DPoser
        if not isinstance(body_model, SMPLX):
            raise TypeError(f"SMPLify fits the SMPL-X wrapper of body_model.smpl (49 mapped joints), got {type(body_model).__name__}")
        self.smpl = body_model
        self.device = args.device
        self.focal_length = focal_length
        self.step_size = step_size
        # the confidences of these joints are zeroed before the body stage (smplify.py:137-139)
        self.ign_joints = [constants.JOINT_IDS[i] for i in ["OP Neck", "OP RHip", "OP LHip", "Right Hip", "Left Hip"]]
        self.num_iters = num_iters
        self.batch_size = batch_size
        self.pose_prior = pose_prior if pose_prior is not None else DPoser(batch_size, args.config_path, args)
        self.sde_N = args.sde_N
        self.time_strategy = args.time_strategy
        self.sample_time = round(args.sde_N * 0.9)           # smplify.py:143
        self.sample_trun = 20.0
        self.loss_weights = {"pose_prior_weight": [50, 20, 10, 5, 2], "shape_prior_weight": [50, 20, 10, 5, 2],
                             "angle_prior_weight": [150, 50, 30, 15, 5]}          # smplify.py:145-149
        self.stages = len(self.loss_weights["pose_prior_weight"])
        self._calls = 0

    # ---- time schedule (smplify.py:151-166)
    def sample_discrete_time(self, iteration):
        total_steps = self.stages * self.num_iters
        if self.time_strategy == "1":
            return int(torch.randint(self.sde_N, [1]))        # torch's host generator, one draw per call as the reference
        if self.time_strategy == "2":
            return int(self.sample_time)
        if self.time_strategy == "3":
            # torch.tensor(int) * float is float32 arithmetic (the form of tasks.motion_denoising.MotionDenoise._quan_t)
            f = np.float32(total_steps - iteration - 1) * np.float32(self.sde_N / (self.sample_trun * total_steps))
            return int(self.sde_N - math.floor(float(f)) - 5)
        raise NotImplementedError

    def time_table(self):
        """quan_t of every body iteration, then the one the reference draws for the final reprojection loss (smplify.py:274)."""
        quan = [self.sample_discrete_time(i) for i in range(self.stages * self.num_iters)]
        return quan, self.sample_discrete_time(self.num_iters - 1)

    def _stage_weights(self):
        return [dict(zip(self.loss_weights.keys(), vals)) for vals in zip(*self.loss_weights.values())]

    def fused_supported(self):
        """The one host predicate: configurations the one-call loop covers."""
        from ..algorithms.advanced.model import ScoreModelFC
        p = self.pose_prior
        nz = p.Normalizer
        return (sde_lib.sde_desc(p.sde, bool(getattr(p, "continuous", True))) is not None and isinstance(p.model, ScoreModelFC)
                and getattr(nz, "rot_rep", None) in ("axis", "rot6d") and _sub_mesh(self.smpl) is not None
                and self.time_strategy in ("1", "2", "3"))

    def __call__(self, init_pose, init_betas, init_cam_t, camera_center, keypoints_2d, fused=True, noise=None, seed=None):
        B = init_pose.shape[0]
        if fused and not self.fused_supported():
            raise NotImplementedError("the one-call SMPLify loop covers sub-VP / VP / VE score networks (continuous or discrete), axis-angle / "
                                      "rot6d normalisers and a joint map without landmark rows; use fused=False")
        quan, _ = self.time_table()
        ts = self.pose_prior.timesteps
        t_list = [float(ts[q]) for q in quan]
        if fused:
            return self._call_fused(init_pose, init_betas, init_cam_t, camera_center, keypoints_2d, t_list, noise, seed)
        return self._call_stepwise(init_pose, init_betas, init_cam_t, camera_center, keypoints_2d, quan, noise)

    # ---- step by step (smplify.py:182-281 as written): the repository's SMPLX, autograd, torch.optim.Adam
    def _call_stepwise(self, init_pose, init_betas, init_cam_t, camera_center, keypoints_2d, quan, noise):
        camera_translation = init_cam_t.clone()
        joints_2d = keypoints_2d[:, :, :2]
        joints_conf = keypoints_2d[:, :, -1]                  # a view: the zeroing below reaches the caller (smplify.py:238)
        body_pose = init_pose[:, 3:].detach().clone()
        global_orient = init_pose[:, :3].detach().clone()
        betas = init_betas.detach().clone()
        global_orient.requires_grad = True
        camera_translation.requires_grad = True
        opt = torch.optim.Adam([global_orient, camera_translation], lr=self.step_size, betas=(0.9, 0.999))
        for _ in range(self.num_iters):
            out = self.smpl(betas=betas, body_pose=body_pose, global_orient=global_orient, pose2rot=True, transl=camera_translation)
            loss = camera_fitting_loss(out.joints, camera_translation, init_cam_t, camera_center, joints_2d, joints_conf,
                                       focal_length=self.focal_length)
            opt.zero_grad()
            loss.backward()
            opt.step()
        camera_translation.requires_grad = False
        body_pose.requires_grad = True
        betas.requires_grad = True
        joints_conf[:, self.ign_joints] = 0.
        opt = torch.optim.Adam([body_pose, betas, global_orient], lr=self.step_size, betas=(0.9, 0.999))
        k = 0
        for current_weights in self._stage_weights():
            for _ in range(self.num_iters):
                out = self.smpl(betas=betas, body_pose=body_pose, global_orient=global_orient, pose2rot=True, transl=camera_translation)
                z = None if noise is None else noise[k]
                prior = lambda bp, bt, q, z=z: self._prior_stepwise(bp, q, z)
                loss = body_fitting_loss(body_pose, betas, out.joints, camera_translation, camera_center, joints_2d, joints_conf, prior,
                                         quan_t=quan[k], focal_length=self.focal_length, **current_weights, verbose=False)
                opt.zero_grad()
                loss.backward()
                opt.step()
                k += 1
        with torch.no_grad():
            out = self.smpl(betas=betas, body_pose=body_pose, global_orient=global_orient, pose2rot=True, transl=camera_translation)
            reprojection_loss = body_fitting_loss(body_pose, betas, out.joints, camera_translation, camera_center, joints_2d, joints_conf,
                                                  None, quan_t=0, focal_length=self.focal_length, output="reprojection", verbose=False)
        pose = torch.cat([global_orient, body_pose], dim=-1).detach()
        return pose, betas.detach(), camera_translation, reprojection_loss

    def _prior_stepwise(self, body_pose, quan_t, z):
        """DPoser.forward (smplify.py:109-115) with a gradient path to the axis-angle pose also under rot_rep = 'rot6d' (the HIP
        axis-angle -> 6-D conversion behind Posenormalizer.offline_normalize has no backward; the reference's torch conversion has)."""
        from ..dataset.AMASS import N_POSES
        from .motion_denoising import _normalize_with_grad
        p = self.pose_prior
        x = _normalize_with_grad(p.Normalizer, body_pose[:, :N_POSES * 3])
        return p.DPoser_loss(x, float(p.timesteps[int(quan_t)]), z=z)

    # ---- one C call per group of images
    def _call_fused(self, init_pose, init_betas, init_cam_t, camera_center, keypoints_2d, t_list, noise, seed, group_cap=None):
        B = init_pose.shape[0]
        dev = init_pose.device
        _C.require_gpu(init_pose, "SMPLify input")
        f32 = lambda x: x.detach().to(dev, torch.float32).contiguous()
        sub, sub_map = _sub_mesh(self.smpl)
        core = sub
        L, nb = core.num_betas + core.num_expression_coeffs, core.num_betas
        orient = f32(init_pose[:, :3]).clone()
        body = f32(init_pose[:, 3:]).clone()
        shape = torch.zeros(B, L, dtype=torch.float32, device=dev)
        shape[:, :init_betas.shape[1]] = f32(init_betas)
        cam_t = f32(init_cam_t).clone()
        cam_est = f32(init_cam_t)
        kp = f32(keypoints_2d).clone()
        fl = self.focal_length
        focal = (f32(fl).reshape(-1).expand(B).contiguous() if torch.is_tensor(fl) else torch.full((B,), float(fl), device=dev))
        center = f32(camera_center)
        reproj = torch.empty(B, kp.shape[1], dtype=torch.float32, device=dev)
        p = self.pose_prior
        model, nz = p.model, p.Normalizer
        n_body = len(t_list)
        net = ScoreNetCall(model, p.sde, bool(getattr(p, "continuous", True)), None, max(1, n_body), dev)      # (its workspace: per group, below)
        rot6d = getattr(nz, "rot_rep", "axis") == "rot6d"
        Dn = net.eng.D
        if noise is not None and tuple(noise.shape) != (n_body, B, Dn):
            raise _C.DPoserHipError(f"noise must be [n_stages * num_iters, B, network inputs] = {(n_body, B, Dn)}, got {tuple(noise.shape)}")
        mode, na, nbv = normalizer_tables(nz, body)
        # keypoint rows of the sub core's joint output: each row's keypoints in map order (the kernels sum them without atomics)
        tables = BodyTables(core)
        rows = tables.rows
        m = sub_map.numpy()
        order = np.argsort(m, kind="stable")
        ptr = np.zeros(rows + 1, np.int32)
        np.add.at(ptr, m + 1, 1)
        ptr = np.cumsum(ptr).astype(np.int32)
        jmap_d = sub_map.to(dev)
        ptr_d = torch.tensor(ptr, device=dev)
        ent_d = torch.tensor(order.astype(np.int32), device=dev)
        fold = core.joint_fold_tables()
        ids = lambda names_: [constants.JOINT_IDS[n] for n in names_]
        op, gt = ids(["OP RHip", "OP LHip", "OP RShoulder", "OP LShoulder"]), ids(["Right Hip", "Left Hip", "Right Shoulder", "Left Shoulder"])
        ign = list(self.ign_joints) + [0] * (8 - len(self.ign_joints))
        wts = self.loss_weights
        seed_v = int(model._rng_seed + 17 if seed is None else seed)
        step0 = p._calls + 1
        p._calls += n_body
        lib = _C.lib()
        cap = group_cap or _MAX_PER_CALL
        self.loss_log = torch.zeros(self.num_iters * (1 + self.stages), B, 4, dtype=torch.float32, device=dev)
        logs = []
        for g0 in range(0, B, cap):
            g1 = min(B, g0 + cap)
            Bg = g1 - g0
            sl = slice(g0, g1)
            net.workspace(Bg)
            body_fields = tables.fields(Bg, dev)
            scratch = torch.empty(int(lib.dposer_smplify_scratch_bytes(Bg, core.V, core.J, rows, L, Dn)), dtype=torch.uint8, device=dev)
            log = torch.zeros(self.num_iters * (1 + self.stages), Bg, 4, dtype=torch.float32, device=dev)
            views = [t[sl] for t in (orient, body, shape, cam_t, kp, reproj)]
            grp = [v if g0 == 0 and g1 == B else v.contiguous() for v in views]
            nzs = None if noise is None else f32(noise[:, sl])
            focal_g, center_g, est_g = focal[sl].contiguous(), center[sl].contiguous(), cam_est[sl].contiguous()
            a = _C.SmplifyArgs(
                **net.fields(), **body_fields,
                v_template=_C.ptr(core.v_template), shapedirs=_C.ptr(core.shapedirs), j_template=_C.ptr(core.j_template), jdirs=_C.ptr(core.jdirs),
                fold=C.pointer(fold[0]), orient_segment=tables.segment("global_orient"), num_shape=L, num_betas=nb, batch=Bg, row0=g0, inv_batch=1.0 / B,
                n_keypoints=int(kp.shape[1]), joint_map=_C.ptr(jmap_d), map_ptr=_C.ptr(ptr_d), map_entry=_C.ptr(ent_d),
                op_joints=(C.c_int32 * 4)(*op), gt_joints=(C.c_int32 * 4)(*gt), ign_joints=(C.c_int32 * 8)(*ign), n_ign=len(self.ign_joints),
                keypoints=_C.ptr(grp[4]), focal_length=_C.ptr(focal_g), camera_center=_C.ptr(center_g),
                cam_t_est=_C.ptr(est_g), global_orient=_C.ptr(grp[0]), body_pose=_C.ptr(grp[1]), shape=_C.ptr(grp[2]),
                cam_t=_C.ptr(grp[3]), norm_mode=mode, norm_a=_C.ptr(na), norm_b=_C.ptr(nbv), rot6d=1 if rot6d else 0, num_iters=self.num_iters,
                n_stages=self.stages, t_host=float_array(t_list), w_pose_host=float_array(wts["pose_prior_weight"]), w_shape_host=float_array(wts["shape_prior_weight"]),
                w_angle_host=float_array(wts["angle_prior_weight"]), sigma=100.0, depth_weight=100.0, lr=float(self.step_size), beta1=0.9, beta2=0.999,
                eps=1e-8, seed=seed_v, step0=int(step0) & 0xFFFFFFFF, noise=_C.ptr(nzs), scratch=_C.ptr(scratch), loss_log=_C.ptr(log),
                reprojection=_C.ptr(grp[5]))
            _C.check(lib.dposer_smplify_optimize(C.byref(a), _C.stream_ptr()), "dposer_smplify_optimize")
            for v, gv in zip(views, grp):
                if v is not gv:
                    v.copy_(gv)
            logs.append(log)
        self.loss_log = logs[0] if len(logs) == 1 else torch.cat(logs, dim=1)
        # joints_conf[:, ign_joints] = 0 writes through a view into the caller's keypoints (smplify.py:133,238)
        keypoints_2d[:, :, -1].copy_(kp[:, :, -1].to(keypoints_2d.device, keypoints_2d.dtype))
        pose = torch.cat([orient, body], dim=-1)
        return pose, shape[:, :init_betas.shape[1]].clone(), cam_t, reproj
