"""BodyModel -- counterpart of the reference's lib/body_model/body_model.py:8-112 (a wrapper over
``smplx.{SMPL,SMPLH,SMPLX}``).  smplx is an un-vendored dependency of the reference; here the model
arithmetic (Rodrigues, kinematic chain, pose-blend GEMM, skinning, landmark joints -- smplx/lbs.py)
runs in the HIP kernels of dposer_amd/csrc/fk.hip behind ``dposer_fk_joints`` / ``dposer_lbs_forward``.

``bm_path`` may be an official model file (``.npz`` / ``.pkl``) or directory (``body_model/assets.py``), or an asset dictionary
(``body_model.synthetic.make_synthetic_asset``).
``model_type`` 'smpl' (24 joints), 'smplh' (52) and 'smplx' (55) share the kernels: the C library unrolls the kinematic chain
over the matching compile-time parents table.
"""
import ctypes as C

import numpy as np
import torch
import torch.nn as nn

from .. import _C
from .synthetic import load_model_npz, load_smplx_npz  # noqa: F401


class Struct:
    """smplx.utils.Struct: attribute bag."""

    def __init__(self, **kwargs):
        for k, v in kwargs.items():
            setattr(self, k, v)


# full_pose order of smplx.{SMPL,SMPLH,SMPLX}.forward (body_models.py): which keyword feeds which joints
_SEGMENTS = {
    "smpl": (("global_orient", 1), ("body_pose", 23)),
    "smplh": (("global_orient", 1), ("body_pose", 21), ("left_hand_pose", 15), ("right_hand_pose", 15)),
    "smplx": (("global_orient", 1), ("body_pose", 21), ("jaw_pose", 1), ("leye_pose", 1), ("reye_pose", 1),
              ("left_hand_pose", 15), ("right_hand_pose", 15)),
}
_SMPLX_SEGMENTS = _SEGMENTS["smplx"]
_MAX_SEG = 7


class _ShapeBlendFunction(torch.autograd.Function):
    """dposer_shape_blend_forward / _backward: (shape [B, L]) -> (v_shaped [B, V, 3], j_rest [B, J, 3])."""

    @staticmethod
    def forward(ctx, core, shape):
        B, L = shape.shape
        dev = shape.device
        sh = shape.detach().contiguous().float()
        vs = torch.empty(B, core.V, 3, dtype=torch.float32, device=dev)
        jr = torch.empty(B, core.J, 3, dtype=torch.float32, device=dev)
        _C.check(_C.lib().dposer_shape_blend_forward(_C.ptr(core.v_template), _C.ptr(core.shapedirs), _C.ptr(core.j_template), _C.ptr(core.jdirs),
                                                     _C.ptr(sh), _C.ptr(vs), _C.ptr(jr), core.V, core.J, L, B, _C.stream_ptr()),
                 "dposer_shape_blend_forward")
        ctx.core, ctx.B, ctx.L = core, B, L
        return vs, jr

    @staticmethod
    def backward(ctx, d_vs, d_jr):
        core, B, L = ctx.core, ctx.B, ctx.L
        lib = _C.lib()
        dv = d_vs.contiguous().float()
        dj = d_jr.contiguous().float()
        out = torch.empty(B, L, dtype=torch.float32, device=dv.device)
        scratch = torch.empty(lib.dposer_shape_blend_scratch_floats(core.V, L, B), dtype=torch.float32, device=dv.device)
        _C.check(lib.dposer_shape_blend_backward(_C.ptr(core.shapedirs), _C.ptr(core.jdirs), _C.ptr(dv), _C.ptr(dj), _C.ptr(out), _C.ptr(scratch),
                                                 core.V, core.J, L, B, _C.stream_ptr()), "dposer_shape_blend_backward")
        return None, out


def _marshal_segments(core, segs, B):
    """The pose segments of one call as the C ABI takes them: (device pointers [_MAX_SEG], joint counts [_MAX_SEG], the detached
    contiguous fp32 tensors behind the pointers -- None where a segment is absent).  ``segs`` is in ``core.segments`` order."""
    segp = (C.c_void_p * _MAX_SEG)()
    segj = (C.c_int32 * _MAX_SEG)()
    keep = []
    for i, ((_, nj), t) in enumerate(zip(core.segments, segs)):
        segj[i] = nj
        if t is not None:
            t = t.detach().reshape(B, nj * 3).contiguous().float()
            keep.append(t)
            segp[i] = t.data_ptr()
        else:
            keep.append(None)
            segp[i] = None
    return segp, segj, keep


class _LBSFunction(torch.autograd.Function):
    """dposer_lbs_forward / dposer_lbs_backward as one differentiable op.
    inputs: core, n_seg_tensors..., v_shaped, j_rest, transl (any may be None)."""

    @staticmethod
    def forward(ctx, core, batched, v_shaped, j_rest, transl, *segs):
        B = next(t for t in segs if t is not None).shape[0] if any(t is not None for t in segs) else (transl.shape[0] if transl is not None else v_shaped.shape[0])
        dev = core.v_template.device
        h, lib = core._handle(), _C.lib()
        ws = torch.empty(lib.dposer_lbs_workspace_bytes(h, B), dtype=torch.uint8, device=dev)     # private: read back in backward
        nseg = len(core.segments)
        segp, segj, keep = _marshal_segments(core, segs, B)
        vs, jr = v_shaped.detach().contiguous(), j_rest.detach().contiguous()
        tr = None if transl is None else transl.detach().contiguous().float()
        verts = torch.empty(B, core.V, 3, dtype=torch.float32, device=dev)
        joints = torch.empty(B, core.J + core.n_extra + core.n_lmk, 3, dtype=torch.float32, device=dev)
        _C.check(lib.dposer_lbs_forward(h, _C.ptr(ws), _C.ptr(core._packed_posedirs()), segp, segj, nseg, _C.ptr(jr), 1 if batched else 0,
                                        _C.ptr(vs), 1 if batched else 0, _C.ptr(core.skin_idx), _C.ptr(core.skin_w),
                                        int(core.skin_idx.shape[1]), _C.ptr(tr), _C.ptr(core.extra_vertex_ids), _C.ptr(core.lmk_tri),
                                        _C.ptr(core.lmk_bary_coords), _C.ptr(verts), _C.ptr(joints), B, _C.stream_ptr()),
                 "dposer_lbs_forward")
        ctx.core, ctx.batched, ctx.ws, ctx.keep, ctx.vs, ctx.jr, ctx.B = core, batched, ws, keep, vs, jr, B
        ctx.has_transl = transl is not None
        ctx.seg_given = [t is not None for t in segs]
        return verts, joints

    @staticmethod
    def backward(ctx, d_verts, d_joints):
        core, B = ctx.core, ctx.B
        dev = d_verts.device
        h, lib = core._handle(), _C.lib()
        J = core.J
        dv = d_verts.contiguous().float()
        dj = d_joints.contiguous().float()
        # extras / landmarks are gathers of vertices (smplx VertexJointSelector / vertices2landmarks): their gradients d_joints[:, J:] belong to
        # the <= 21 + 3 * 51 vertices they read.  dposer_lbs_backward_fold adds them INSIDE the library (k_fold_rows writes the corrected
        # rows into its workspace, the skinning kernels read those instead of the caller's rows; fixed summation order): the incoming
        # gradient is only read -- rounds 2-4 did this here with torch.matmul (hipBLASLt) + index / index_put launches and wrote into
        # autograd's tensor in place, restoring it afterwards.
        return _LBSFunction._backward_body(ctx, core, B, dev, h, lib, J, dv, dj)

    @staticmethod
    def _backward_body(ctx, core, B, dev, h, lib, J, dv, dj):
        # transl shifts every vertex and every joint row (the weights of an extra joint / landmark over its vertices sum to 1)
        d_transl = (dv.sum(dim=1) + dj.sum(dim=1)) if ctx.has_transl else None
        ws_b = torch.empty(lib.dposer_lbs_backward_workspace_bytes(h, B), dtype=torch.uint8, device=dev)
        segp, dsegp = (C.c_void_p * _MAX_SEG)(), (C.c_void_p * _MAX_SEG)()
        segj = (C.c_int32 * _MAX_SEG)()
        dsegs = []
        for i, ((_, nj), t) in enumerate(zip(core.segments, ctx.keep)):
            segj[i] = nj
            segp[i] = None if t is None else t.data_ptr()
            if t is not None:
                g = torch.empty_like(t)
                dsegs.append(g)
                dsegp[i] = g.data_ptr()
            else:
                dsegs.append(None)
                dsegp[i] = None
        # gradients w.r.t. the rest shape only when it is differentiable (betas / expression being optimised): d v_posed alone is a
        # 515 MB stream at 4096 poses
        need_vs, need_jr = ctx.needs_input_grad[2], ctx.needs_input_grad[3]
        d_jrest = torch.empty(B, J, 3, dtype=torch.float32, device=dev) if need_jr else None
        d_vposed = torch.empty(B, core.V, 3, dtype=torch.float32, device=dev) if need_vs else None
        jptr, jvidx, jw = core.joint_csr()
        fold = core.joint_fold_tables() if (core.n_extra + core.n_lmk) and dj.shape[1] > J else None
        _C.check(lib.dposer_lbs_backward_fold(h, _C.ptr(ctx.ws), _C.ptr(ws_b), _C.ptr(core._packed_posedirs_bwd()), segp, segj, len(core.segments), _C.ptr(ctx.jr),
                                              1 if ctx.batched else 0, _C.ptr(ctx.vs), 1 if ctx.batched else 0, _C.ptr(core.skin_idx),
                                              _C.ptr(core.skin_w), int(core.skin_idx.shape[1]), _C.ptr(jptr), _C.ptr(jvidx), _C.ptr(jw), _C.ptr(dv),
                                              _C.ptr(dj), dj.shape[1] * 3, None if fold is None else C.byref(fold[0]), dsegp, _C.ptr(d_jrest),
                                              _C.ptr(d_vposed), B, _C.stream_ptr()),
                 "dposer_lbs_backward_fold")
        if ctx.batched:
            g_vs, g_jr = d_vposed, d_jrest
        else:
            g_vs = None if d_vposed is None else d_vposed.sum(dim=0)
            g_jr = None if d_jrest is None else d_jrest.sum(dim=0)
        return (None, None, g_vs, g_jr, d_transl, *dsegs)


class _FKJointsFunction(torch.autograd.Function):
    """dposer_fk_joints / dposer_fk_joints_backward as one differentiable op: posed joints [B, n_out, 3] whose gradient is the chain
    rule over those joints alone (no vertices, no skinning, no blend GEMM -- what ``_LBSFunction`` pays for the same numbers).
    inputs: core, batched, j_rest, transl (or None), n_out, the pose segments in ``core.segments`` order (any may be None)."""

    @staticmethod
    def forward(ctx, core, batched, j_rest, transl, n_out, *segs):
        B = next(t for t in segs if t is not None).shape[0] if any(t is not None for t in segs) else (transl.shape[0] if transl is not None else j_rest.shape[0])
        dev = core.v_template.device
        h, lib = core._handle(), _C.lib()
        segp, segj, keep = _marshal_segments(core, segs, B)
        jr = j_rest.detach().contiguous().float()
        tr = None if transl is None else transl.detach().contiguous().float()
        joints = torch.empty(B, n_out, 3, dtype=torch.float32, device=dev)
        _C.check(lib.dposer_fk_joints(h, segp, segj, len(core.segments), _C.ptr(jr), 1 if batched else 0, _C.ptr(tr), _C.ptr(joints), None, n_out, B,
                                      _C.stream_ptr()), "dposer_fk_joints")
        ctx.core, ctx.batched, ctx.keep, ctx.jr, ctx.B, ctx.n_out = core, batched, keep, jr, B, n_out
        ctx.has_transl = transl is not None
        return joints

    @staticmethod
    def backward(ctx, d_joints):
        core, B, n_out = ctx.core, ctx.B, ctx.n_out
        dev = d_joints.device
        h, lib = core._handle(), _C.lib()
        dj = d_joints.contiguous().float()
        d_transl = dj.sum(dim=1) if ctx.has_transl else None
        segp, dsegp = (C.c_void_p * _MAX_SEG)(), (C.c_void_p * _MAX_SEG)()
        segj = (C.c_int32 * _MAX_SEG)()
        dsegs = []
        for i, ((_, nj), t) in enumerate(zip(core.segments, ctx.keep)):
            segj[i] = nj
            segp[i] = None if t is None else t.data_ptr()
            g = None if t is None or not ctx.needs_input_grad[5 + i] else torch.empty_like(t)
            dsegs.append(g)
            dsegp[i] = None if g is None else g.data_ptr()
        d_jrest = torch.empty(B, n_out, 3, dtype=torch.float32, device=dev) if ctx.needs_input_grad[2] else None
        ws = torch.empty(lib.dposer_fk_joints_backward_workspace_bytes(h, n_out, B), dtype=torch.uint8, device=dev)
        _C.check(lib.dposer_fk_joints_backward(h, segp, segj, len(core.segments), _C.ptr(ctx.jr), 1 if ctx.batched else 0, _C.ptr(dj), n_out * 3,
                                               n_out, dsegp, _C.ptr(d_jrest), _C.ptr(ws), B, _C.stream_ptr()), "dposer_fk_joints_backward")
        g_jr = None
        if d_jrest is not None:                      # rest joints >= n_out move no evaluated joint
            if not ctx.batched:
                d_jrest = d_jrest.sum(dim=0)
            g_jr = torch.nn.functional.pad(d_jrest, (0, 0, 0, core.J - n_out))
        return (None, None, g_jr, d_transl, None, *dsegs)


class _SMPLCore(nn.Module):
    """What the reference reaches as ``BodyModel.bm`` (an smplx.SMPL / SMPLH / SMPLX instance): buffers + forward.
    ``model_type`` selects the full-pose layout (``_SEGMENTS``); expression coefficients and landmarks exist for SMPL-X only."""
    NUM_HAND_JOINTS = 15

    def __init__(self, asset, num_betas=10, num_expression_coeffs=10, batch_size=1, model_type="smplx"):
        super().__init__()
        self.batch_size = batch_size
        self.model_type = model_type
        self.segments = _SEGMENTS[model_type]
        self.NUM_BODY_JOINTS = dict(self.segments)["body_pose"]
        self.NUM_JOINTS = sum(n for _, n in self.segments) - 1          # smplx's class constant: joints without the root
        a = asset
        self.num_betas = num_betas
        self.num_expression_coeffs = num_expression_coeffs if model_type == "smplx" else 0
        f32 = lambda x: torch.tensor(np.asarray(x), dtype=torch.float32)
        self.register_buffer("v_template", f32(a["v_template"]))
        self.register_buffer("shapedirs", f32(a["shapedirs"]))                  # [V,3,betas+expr]
        self.register_buffer("posedirs", f32(a["posedirs"]))                    # [486, V*3]
        self.register_buffer("J_regressor", f32(a["J_regressor"]))
        self.register_buffer("lbs_weights", f32(a["weights"]))
        self.register_buffer("parents", torch.tensor(np.asarray(a["parents"]), dtype=torch.long))
        self.register_buffer("faces_tensor", torch.tensor(np.asarray(a["faces"]).astype(np.int64), dtype=torch.long))
        self.register_buffer("lmk_faces_idx", torch.tensor(np.asarray(a["lmk_faces_idx"]).astype(np.int64)))
        self.register_buffer("lmk_bary_coords", f32(np.asarray(a["lmk_bary_coords"]).reshape(-1, 3)))
        self.register_buffer("extra_vertex_ids", torch.tensor(np.asarray(a["extra_joint_vertex_ids"]).astype(np.int32)))
        # ELL form of the skinning weights
        w = np.asarray(a["weights"], dtype=np.float32)
        k = int((w != 0).sum(axis=1).max())
        order = np.argsort(-(w != 0).astype(np.int8), axis=1, kind="stable")[:, :k]
        if k != 4:
            # every fast skinning path (runs of poses, the matrix-pipe backward, the fused temporal gradient) is built for the ELL width 4 of
            # the SMPL-family templates; other widths run the general kernels -- correct (tests/test_gpu_assets.py: 5 and 8), slower
            import warnings
            warnings.warn(f"body model asset has up to {k} skinning influences per vertex (SMPL-family templates have 4): the general LBS kernels "
                          "are used -- same results, several times slower forward and backward", RuntimeWarning, stacklevel=3)
        self.register_buffer("skin_idx", torch.tensor(order.astype(np.int32)))
        self.register_buffer("skin_w", torch.tensor(np.take_along_axis(w, order, axis=1)))
        tri = np.asarray(a["faces"])[np.asarray(a["lmk_faces_idx"]).astype(np.int64)].reshape(-1, 3)
        self.register_buffer("lmk_tri", torch.tensor(tri.astype(np.int32)))
        self.J, self.V = int(w.shape[1]), int(w.shape[0])
        if self.J != self.NUM_JOINTS + 1:
            raise ValueError(f"model_type {model_type!r} has {self.NUM_JOINTS + 1} joints, the asset has {self.J}")
        self.n_extra, self.n_lmk = int(len(a["extra_joint_vertex_ids"])), int(len(a["lmk_faces_idx"]))
        L = self.num_betas + self.num_expression_coeffs
        if self.shapedirs.shape[2] != L:
            raise ValueError(f"asset has {self.shapedirs.shape[2]} shape directions, expected num_betas + num_expression_coeffs = {L}")
        # joint regression is linear: apply it to the template and to every blend-shape direction once (dposer_shape_blend_*)
        self.register_buffer("j_template", (self.J_regressor @ self.v_template).contiguous())                       # [J, 3]
        self.register_buffer("jdirs", torch.einsum("jv,vkl->jkl", self.J_regressor, self.shapedirs).contiguous())   # [J, 3, L]
        # the kernels gather vertices through these index tables without bounds checks
        ids = np.asarray(a["extra_joint_vertex_ids"])
        if ids.size and (ids.min() < 0 or ids.max() >= self.V):
            raise ValueError(f"extra_joint_vertex_ids must lie in [0, {self.V}): got [{ids.min()}, {ids.max()}]")
        if tri.size and (tri.min() < 0 or tri.max() >= self.V):
            raise ValueError(f"landmark faces reference vertices outside [0, {self.V})")
        self._parents_np = np.asarray(a["parents"]).astype(np.int32)
        self._h = None
        self._posedirs_packed = None
        self._ws = None
        self._rest_cache = {}
        self._zero_cache = {}

    # ---- engine ----
    def _handle(self):
        if self._h is None:
            desc = _C.BodyDesc(self.J, self.V, self.num_betas + self.num_expression_coeffs, self.n_extra, self.n_lmk)
            h = C.c_void_p()
            par = (C.c_int32 * self.J)(*[int(p) for p in self._parents_np])
            _C.check(_C.lib().dposer_body_create(C.byref(desc), par, C.byref(h)), "dposer_body_create")
            self._h = h
        return self._h

    def __del__(self):
        # the C handle owns device tables (joint lists, weight fragments) and the side streams / events of the backward: release them with
        # the module (round 6: they used to live until the process ended -- a test session built ~100 body models)
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                _C.lib().dposer_body_destroy(h)
            except Exception:      # (interpreter shutdown: the library may already be gone)
                pass
            self._h = None

    def joint_csr(self):
        """CSR-by-joint form of the skinning weights (which vertices does joint j move) for the backward kernel."""
        if getattr(self, "_jcsr", None) is None or self._jcsr[0].device != self.skin_idx.device:
            idx, w = self.skin_idx.cpu().numpy(), self.skin_w.cpu().numpy()
            v = np.repeat(np.arange(idx.shape[0], dtype=np.int32), idx.shape[1])
            j, ww = idx.reshape(-1), w.reshape(-1)
            nz = ww != 0
            v, j, ww = v[nz], j[nz], ww[nz]
            order = np.argsort(j, kind="stable")
            ptr = np.zeros(self.J + 1, dtype=np.int32)
            np.add.at(ptr, j + 1, 1)
            ptr = np.cumsum(ptr).astype(np.int32)
            dev = self.skin_idx.device
            self._jcsr = (torch.tensor(ptr, device=dev), torch.tensor(v[order].astype(np.int32), device=dev),
                          torch.tensor(ww[order].astype(np.float32), device=dev))
            if dev.type == "cuda":
                # setup call (synchronises, allocates): the re-cut table the streaming joint-gradient kernel of dposer_lbs_backward
                # walks lives in the handle; built here, once per (lists, device), never inside the backward call
                _C.check(_C.lib().dposer_lbs_prepare_joint_lists(self._handle(), _C.ptr(self._jcsr[0]), _C.ptr(self._jcsr[1]),
                                                                 _C.ptr(self._jcsr[2]), _C.stream_ptr()), "dposer_lbs_prepare_joint_lists")
        return self._jcsr

    def joint_fold_tables(self):
        """(dposer_lbs_joint_fold struct, tensors it points at) for dposer_lbs_backward_fold, built once per (asset, device): the vertices
        the vertex-selected extra joints and the barycentric landmarks read, each with its (d_joints row, weight) entries -- extras
        first, then landmarks in landmark order: the order the library adds them in."""
        dev = self.skin_idx.device
        if getattr(self, "_jfold_tab", None) is None or self._jfold_tab[1][0].device != dev:
            ex = self.extra_vertex_ids.cpu().numpy().astype(np.int64)
            tri = self.lmk_tri.cpu().numpy().astype(np.int64).reshape(-1, 3)
            bary = self.lmk_bary_coords.cpu().numpy().astype(np.float32).reshape(-1, 3)
            per = {}
            for e, v in enumerate(ex):
                per.setdefault(int(v), []).append((self.J + e, 1.0))
            for l in range(len(tri)):
                for f in range(3):
                    per.setdefault(int(tri[l, f]), []).append((self.J + len(ex) + l, float(bary[l, f])))
            uniq = sorted(per)
            vslot = np.full(self.V, -1, dtype=np.int32)
            ptr, rows, ws = [0], [], []
            for u, v in enumerate(uniq):
                vslot[v] = u
                for r, w in per[v]:
                    rows.append(r)
                    ws.append(w)
                ptr.append(len(rows))
            t = (torch.tensor(vslot, device=dev), torch.tensor(np.asarray(uniq, dtype=np.int32), device=dev),
                 torch.tensor(np.asarray(ptr, dtype=np.int32), device=dev), torch.tensor(np.asarray(rows, dtype=np.int32), device=dev),
                 torch.tensor(np.asarray(ws, dtype=np.float32), device=dev))
            st = _C.LbsJointFold(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), t[4].data_ptr(), len(uniq))
            self._jfold_tab = (st, t)
        return self._jfold_tab

    def _packed_posedirs_bwd(self):
        dev = self.posedirs.device
        if getattr(self, "_posedirs_bwd", None) is None or self._posedirs_bwd.device != dev:
            h = self._handle()
            self._posedirs_bwd = torch.empty(_C.lib().dposer_lbs_posedirs_bwd_packed_bytes(h), dtype=torch.uint8, device=dev)
            _C.check(_C.lib().dposer_lbs_pack_posedirs_bwd(h, _C.ptr(self.posedirs), _C.ptr(self._posedirs_bwd), _C.stream_ptr()),
                     "dposer_lbs_pack_posedirs_bwd")
        return self._posedirs_bwd

    def _packed_posedirs(self):
        dev = self.posedirs.device
        if self._posedirs_packed is None or self._posedirs_packed.device != dev:
            h = self._handle()
            n = _C.lib().dposer_lbs_posedirs_packed_bytes(h)
            self._posedirs_packed = torch.empty(n, dtype=torch.uint8, device=dev)
            _C.check(_C.lib().dposer_lbs_pack_posedirs(h, _C.ptr(self.posedirs), _C.ptr(self._posedirs_packed), _C.stream_ptr()),
                     "dposer_lbs_pack_posedirs")
        return self._posedirs_packed

    def rest_shape(self, betas, expression):
        """v_shaped = v_template + blend_shapes(shape), J = J_regressor @ v_shaped (smplx lbs.py) -> (v_shaped, j_rest, batched).

        * no betas / expression: the template (shared by the whole batch, nothing computed);
        * otherwise ``dposer_shape_blend_forward`` (HIP; differentiable w.r.t. betas / expression through
          ``dposer_shape_blend_backward``).  The task loops pass the SAME constant betas tensor every step
          (motion_denoising.py:64,217: ``self.betas``), so the result is cached on (storage, version, shape) of the inputs --
          an unchanged tensor costs no launch and no host sync; a tensor that requires grad is never cached.  The cache entry
          keeps the input tensors alive, so a freed-and-recycled address can never alias an old entry; writes through raw
          pointers that do not bump ``_version`` are outside the contract (torch ops and ``copy_`` do bump it)."""
        dev = self.v_template.device
        if betas is None and expression is None:
            return self.v_template, self.j_template, False
        B = (betas if betas is not None else expression).shape[0]
        differentiable = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (betas, expression))
        key = None
        if not differentiable:
            key = tuple((t.data_ptr(), t._version, tuple(t.shape), t.dtype) if t is not None else None for t in (betas, expression))
            hit = self._rest_cache.get("shape")
            # the entry holds the input tensors themselves: while it lives their storage cannot be freed and handed to another
            # tensor with the same address and version 0 (the caching allocator does exactly that), and a hit requires the SAME
            # tensor objects' storages, not merely equal addresses
            if hit is not None and hit[0] == key and all(a is b or (a is not None and b is not None and a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr())
                                                         for a, b in zip(hit[3], (betas, expression))):
                return hit[1], hit[2], True
        parts = [betas if betas is not None else torch.zeros(B, self.num_betas, device=dev)]
        if self.num_expression_coeffs:
            parts.append(expression if expression is not None else torch.zeros(B, self.num_expression_coeffs, device=dev))
        elif expression is not None:
            raise ValueError(f"model_type {self.model_type!r} has no expression coefficients")
        shape = torch.cat([t.float() for t in parts], dim=1) if len(parts) > 1 else parts[0].float()
        if shape.shape[1] != self.shapedirs.shape[2]:
            raise ValueError(f"expected {self.shapedirs.shape[2]} shape coefficients, got {shape.shape[1]}")
        v_shaped, j_rest = _ShapeBlendFunction.apply(self, shape)
        if key is not None:
            self._rest_cache["shape"] = (key, v_shaped, j_rest, (betas, expression))
        return v_shaped, j_rest, True

    def forward(self, betas=None, global_orient=None, body_pose=None, left_hand_pose=None, right_hand_pose=None, transl=None,
                expression=None, jaw_pose=None, leye_pose=None, reye_pose=None, return_verts=True, return_full_pose=False,
                joints_only=False, n_joints=None, grad="lbs", **kwargs):
        if grad not in ("lbs", "chain"):
            raise ValueError(f"grad must be 'lbs' or 'chain', got {grad!r}")
        if grad == "chain" and not joints_only:
            raise ValueError("grad='chain' differentiates the posed joints alone: it needs joints_only=True")
        allsegs = dict(global_orient=global_orient, body_pose=body_pose, jaw_pose=jaw_pose, leye_pose=leye_pose, reye_pose=reye_pose,
                       left_hand_pose=left_hand_pose, right_hand_pose=right_hand_pose)
        segs = {name: allsegs[name] for name, _ in self.segments}      # (smplx.SMPL ignores hand / face keywords the same way)
        given = [v for v in list(segs.values()) + [betas, transl, expression] if v is not None]
        if not given:
            raise ValueError("BodyModel.forward needs at least one tensor argument")
        B = given[0].shape[0]
        dev = given[0].device
        _C.require_gpu(given[0], "BodyModel input")
        if B == 0:                  # smplx returns empty outputs for an empty batch; the kernels take B >= 1
            n_out = self.J if n_joints is None else int(n_joints)
            if joints_only:
                return Struct(vertices=None, joints=torch.zeros(0, n_out, 3, dtype=torch.float32, device=dev))
            return self._output(torch.zeros(0, self.V, 3, dtype=torch.float32, device=dev),
                                torch.zeros(0, self.J + self.n_extra + self.n_lmk, 3, dtype=torch.float32, device=dev), segs, betas, expression, B, dev,
                                return_full_pose)
        needs_grad = torch.is_grad_enabled() and any(t.requires_grad for t in given)
        if self.v_template.device != dev:
            raise _C.DPoserHipError("BodyModel buffers and inputs are on different devices; call .to(device)")
        segp = (C.c_void_p * _MAX_SEG)()
        segj = (C.c_int32 * _MAX_SEG)()
        nseg = len(self.segments)
        keep = []
        for i, (name, nj) in enumerate(self.segments):
            t = segs[name]
            segj[i] = nj
            if t is not None:
                t = t.reshape(B, nj * 3).contiguous().float()
                keep.append(t)
                segp[i] = t.data_ptr()
            else:
                segp[i] = None
        v_shaped, j_rest, batched = self.rest_shape(betas, expression)
        tr = None if transl is None else transl.contiguous().float()
        h = self._handle()
        lib = _C.lib()
        if needs_grad and grad == "chain":
            # the chain rule over the queried joints alone (dposer_fk_joints_backward): no vertices are formed in either direction
            n_out = self.J if n_joints is None else int(n_joints)
            return Struct(vertices=None, joints=_FKJointsFunction.apply(self, batched, j_rest, transl, n_out,
                                                                        *[segs[name] for name, _ in self.segments]))
        if needs_grad:
            verts, joints = _LBSFunction.apply(self, batched, v_shaped, j_rest, transl, *[segs[name] for name, _ in self.segments])
            if joints_only:
                return Struct(vertices=None, joints=joints[:, :(self.J if n_joints is None else int(n_joints))])
            return self._output(verts, joints, segs, betas, expression, B, dev, return_full_pose)
        if joints_only:
            n_out = self.J if n_joints is None else int(n_joints)
            joints = torch.empty(B, n_out, 3, dtype=torch.float32, device=dev)
            _C.check(lib.dposer_fk_joints(h, segp, segj, nseg, _C.ptr(j_rest), 1 if batched else 0, _C.ptr(tr), _C.ptr(joints), None, n_out, B,
                                          _C.stream_ptr()), "dposer_fk_joints")
            return Struct(vertices=None, joints=joints)
        need = lib.dposer_lbs_workspace_bytes(h, B)
        if self._ws is None or self._ws.numel() < need or self._ws.device != dev:
            self._ws = torch.empty(need, dtype=torch.uint8, device=dev)
        verts = torch.empty(B, self.V, 3, dtype=torch.float32, device=dev)
        joints = torch.empty(B, self.J + self.n_extra + self.n_lmk, 3, dtype=torch.float32, device=dev)
        _C.check(lib.dposer_lbs_forward(h, _C.ptr(self._ws), _C.ptr(self._packed_posedirs()), segp, segj, nseg, _C.ptr(j_rest),
                                        1 if batched else 0, _C.ptr(v_shaped), 1 if batched else 0, _C.ptr(self.skin_idx),
                                        _C.ptr(self.skin_w), int(self.skin_idx.shape[1]), _C.ptr(tr), _C.ptr(self.extra_vertex_ids),
                                        _C.ptr(self.lmk_tri), _C.ptr(self.lmk_bary_coords), _C.ptr(verts), _C.ptr(joints), B,
                                        _C.stream_ptr()), "dposer_lbs_forward")
        return self._output(verts, joints, segs, betas, expression, B, dev, return_full_pose)

    def lbs_front(self, *, rest=None, betas=None, expression=None, transl=None, **segs):
        """The front half of the LBS forward (``dposer_lbs_forward_front``: FK, skinning transforms, pose-blend offsets) for one batch,
        outside autograd: ``Struct(ws, joints, v_shaped, j_rest, batched, transl, batch)``.  ``ws`` is a fresh workspace holding the
        transforms and the offsets, ``joints [B, J + n_extra + n_lmk, 3]`` has only ``[:, :J]`` written -- what the kernels that skin
        in registers read (``dposer_pose_pair_errors``).  ``segs``: the pose keywords of ``forward``; ``rest``: a
        ``(v_shaped, j_rest, batched)`` triple to use instead of ``rest_shape(betas, expression)``."""
        unknown = set(segs) - {name for name, _ in self.segments}
        if unknown:
            raise ValueError(f"model_type {self.model_type!r} has no pose segments {sorted(unknown)}")
        given = [t for t in segs.values() if t is not None]
        if not given:
            raise ValueError("lbs_front needs at least one pose segment")
        B, dev = int(given[0].shape[0]), given[0].device
        _C.require_gpu(given[0], "BodyModel input")
        if self.v_template.device != dev:
            raise _C.DPoserHipError("BodyModel buffers and inputs are on different devices; call .to(device)")
        with torch.no_grad():
            v_shaped, j_rest, batched = rest if rest is not None else self.rest_shape(betas, expression)
        segp, segj, keep = _marshal_segments(self, [segs.get(name) for name, _ in self.segments], B)
        vs, jr = v_shaped.detach().contiguous(), j_rest.detach().contiguous()
        tr = None if transl is None else transl.detach().contiguous().float()
        h, lib = self._handle(), _C.lib()
        ws = torch.empty(lib.dposer_lbs_workspace_bytes(h, B), dtype=torch.uint8, device=dev)
        joints = torch.empty(B, self.J + self.n_extra + self.n_lmk, 3, dtype=torch.float32, device=dev)
        _C.check(lib.dposer_lbs_forward_front(h, _C.ptr(ws), _C.ptr(self._packed_posedirs()), segp, segj, len(self.segments), _C.ptr(jr),
                                              1 if batched else 0, _C.ptr(tr), _C.ptr(joints), B, _C.stream_ptr()), "dposer_lbs_forward_front")
        return Struct(ws=ws, joints=joints, v_shaped=vs, j_rest=jr, batched=batched, transl=tr, batch=B, segments=keep)

    def _zeros(self, B, n, dev):
        """The all-zero default of a pose segment / betas that was not passed (smplx hands out its own default parameters the same
        way: a shared tensor, not a fresh one).  Cached per (B, n): seven fill launches per call were 34 us of a 0.77 ms forward at
        4096 poses.  Callers must not write into these outputs."""
        key = (B, n, str(dev))
        t = self._zero_cache.get(key)
        if t is None:
            if len(self._zero_cache) > 64:
                self._zero_cache.clear()
            t = self._zero_cache[key] = torch.zeros(B, n, dtype=torch.float32, device=dev)
        return t

    def _output(self, verts, joints, segs, betas, expression, B, dev, return_full_pose):
        """smplx ModelOutput fields (body_models.py): the per-segment poses as given (zeros where the module default applies)."""
        z = lambda n: self._zeros(B, n, dev)
        full = {name: (segs[name].reshape(B, nj * 3) if segs[name] is not None else z(nj * 3)) for name, nj in self.segments}
        return Struct(vertices=verts, joints=joints, betas=betas if betas is not None else z(self.num_betas), expression=expression,
                      global_orient=full["global_orient"], body_pose=full["body_pose"], jaw_pose=full.get("jaw_pose"),
                      left_hand_pose=full.get("left_hand_pose"), right_hand_pose=full.get("right_hand_pose"),
                      full_pose=torch.cat([full[name] for name, _ in self.segments], dim=1) if return_full_pose else None)


_SMPLXCore = _SMPLCore      # (name kept for callers that reach for the SMPL-X core directly)


class BodyModel(nn.Module):
    """lib/body_model/body_model.py:8-112."""

    def __init__(self, bm_path, num_betas=10, batch_size=1, num_expressions=10, model_type="smplx"):
        super().__init__()
        assert model_type in ["smpl", "smplh", "smplx"]                    # body_model.py:39
        if not isinstance(bm_path, dict):
            # a model file or directory (.npz / .pkl; body_model/assets.py restates smplx's loader): the shape / expression spaces
            # are clamped to what the file holds, as smplx does (it prints a warning), and the module is built with the clamped sizes
            asset = load_model_npz(bm_path, model_type, num_betas, num_expressions)
            num_betas, num_expressions = asset["num_betas"], asset["num_expressions"]
        else:
            asset = bm_path
        self.bm = _SMPLCore(asset, num_betas=num_betas, num_expression_coeffs=num_expressions, batch_size=batch_size, model_type=model_type)
        self.num_joints = self.bm.NUM_JOINTS                                # SMPL 23 / SMPL-H 51 / SMPL-X 54 (body_model.py:42,58,62)
        self.model_type = model_type
        self.J_regressor = self.bm.J_regressor.numpy()
        self.J_regressor_idx = {"pelvis": 0, "lwrist": 20, "rwrist": 21, "neck": 12}

    def forward(self, root_orient=None, pose_body=None, pose_hand=None, pose_jaw=None, pose_eye=None, betas=None, trans=None,
                dmpls=None, expression=None, return_dict=False, **kwargs):
        assert dmpls is None
        nh = _SMPLCore.NUM_HAND_JOINTS * 3
        o = self.bm(betas=betas, global_orient=root_orient, body_pose=pose_body,
                    left_hand_pose=None if pose_hand is None else pose_hand[:, :nh],
                    right_hand_pose=None if pose_hand is None else pose_hand[:, nh:],
                    transl=trans, expression=expression, jaw_pose=pose_jaw,
                    leye_pose=None if pose_eye is None else pose_eye[:, :3],
                    reye_pose=None if pose_eye is None else pose_eye[:, 3:], return_full_pose=True, **kwargs)
        out = {"v": o.vertices, "f": self.bm.faces_tensor, "betas": o.betas, "Jtr": o.joints,
               "body_joints": o.joints[:22],        # slices the batch axis, like the reference (body_model.py:95)
               "pose_body": o.body_pose, "full_pose": o.full_pose}
        if self.model_type in ["smplh", "smplx"]:                                        # body_model.py:99-103
            out["pose_hand"] = (self.bm._zeros(o.left_hand_pose.shape[0], 2 * nh, o.left_hand_pose.device) if pose_hand is None
                                else torch.cat([o.left_hand_pose, o.right_hand_pose], dim=-1))
        if self.model_type == "smplx":
            out["pose_jaw"] = o.jaw_pose
            out["pose_eye"] = pose_eye
        return out if return_dict else Struct(**out)

    def lbs_front(self, pose_body, root_orient=None, betas=None, trans=None, rest=None):
        """Front half of ``forward`` for [B, 63] body poses, no vertices and no autograd: see ``_SMPLCore.lbs_front``."""
        return self.bm.lbs_front(rest=rest, betas=betas, transl=trans, global_orient=root_orient, body_pose=pose_body)

    def fk_joints(self, pose_body, root_orient=None, trans=None, n_joints=22, betas=None, grad="lbs"):
        """Joints-only fast path (no vertices): [B, 63] -> [B, n_joints, 3].  Under autograd ``grad="lbs"`` (the default) differentiates
        through the whole LBS forward / backward as before; ``grad="chain"`` through the kinematic chain alone
        (``dposer_fk_joints_backward``): the same gradients for pose, root orientation, translation and betas to fp32 rounding, without
        forming a vertex."""
        return self.bm(betas=betas, global_orient=root_orient, body_pose=pose_body, transl=trans, joints_only=True, n_joints=n_joints,
                       grad=grad).joints
