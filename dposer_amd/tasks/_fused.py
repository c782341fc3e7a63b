"""The prelude the one-call paths share: what a fused C call needs besides its own problem -- the score network's side, the pose
normaliser's tables, the body model's static tables and the host float arrays.  Each object keeps the tensors its pointers reach."""
import ctypes as C

import torch

from .. import _C
from ..algorithms.advanced import sde_lib


class ScoreNetCall:
    """The score-network part of a call with a shared time per step: engine, flat parameters, packed weights (re-packed unless the model
    freezes them), shared-t workspace for ``rows`` samples and ``n_table_rows`` time-table rows, SDE descriptor, ``freq``, ``sigmas``.
    ``rows=None``: no workspace yet -- ``workspace(rows)`` sizes it later (SMPLify: once per group of images)."""

    def __init__(self, model, sde, continuous, rows, n_table_rows, device):
        self.eng = model._engine()
        self.flat = model.flat_params()
        self.packed = self.eng.packed(self.flat, with_backward=False, force=not model.freeze_packed)
        self.n_table_rows, self.device = n_table_rows, device
        self.ws = None if rows is None else self.workspace(rows)
        self.desc = sde_lib.sde_desc(sde, continuous)
        self.freq = self.eng.freq(device, model._fourier_W())
        self.sigmas = model.sigmas

    def workspace(self, rows):
        self.ws = self.eng.workspace(rows, _C.WS_SHARED_T, self.n_table_rows, self.device)
        return self.ws

    def head(self):
        """The leading arguments of the ``dposer_prior_*`` / ``dposer_completion_optimize`` entries."""
        return self.eng.h, _C.ptr(self.flat), _C.ptr(self.packed), _C.ptr(self.ws), C.byref(self.desc)

    def tail(self):
        """Their ``freq, sigmas`` pair."""
        return _C.ptr(self.freq), _C.ptr(self.sigmas)

    def fields(self):
        """The same as the first fields of ``dposer_motion_denoise_args`` / ``dposer_smplify_args``."""
        return dict(net=self.eng.h, flat_params=_C.ptr(self.flat), packed=_C.ptr(self.packed), net_ws=_C.ptr(self.ws), sde=C.pointer(self.desc),
                    freq=_C.ptr(self.freq), sigmas=_C.ptr(self.sigmas))


def normalizer_tables(nz, like):
    """``(mode, a, b)`` of a Posenormalizer for the kernels' normaliser: 0 identity, 1 z-score (mean, std), 2 min-max (min, max); the
    tables flat, contiguous, float32 and on ``like``'s device, or None for mode 0."""
    if not nz.normalize:
        return 0, None, None
    mode, a, b = (2, nz.min_poses, nz.max_poses) if nz.min_max else (1, nz.mean_poses, nz.std_poses)
    return mode, a.to(like.device).reshape(-1).contiguous().float(), b.to(like.device).reshape(-1).contiguous().float()


def float_array(xs):
    """A host ``float[]`` of the values; never of length 0 (an empty schedule still hands C a valid pointer)."""
    vals = [float(x) for x in xs]
    return (C.c_float * max(1, len(vals)))(*vals)


class BodyTables:
    """The static tables of a body-model core as the task structs name them."""

    def __init__(self, core, landmarks=False):
        self.core, self.h, self.landmarks = core, core._handle(), landmarks
        self.names = [name for name, _ in core.segments]
        self.segj = (C.c_int32 * len(self.names))(*[nj for _, nj in core.segments])
        self.jcsr = core.joint_csr()
        self.rows = core.J + core.n_extra + core.n_lmk      # joint rows of the LBS output: tree, extra vertices, landmarks

    def segment(self, name):
        return self.names.index(name)

    def fields(self, batch, device):
        """The struct fields, with the two LBS workspaces for ``batch`` poses (held until the next call of this method)."""
        core, lib = self.core, _C.lib()
        u8 = lambda n: torch.empty(int(n), dtype=torch.uint8, device=device)
        self.ws = u8(lib.dposer_lbs_workspace_bytes(self.h, batch)), u8(lib.dposer_lbs_backward_workspace_bytes(self.h, batch))
        lmk = dict(lmk_tri=_C.ptr(core.lmk_tri), lmk_bary=_C.ptr(core.lmk_bary_coords)) if self.landmarks else {}
        return dict(body=self.h, lbs_ws_fwd=_C.ptr(self.ws[0]), lbs_ws_bwd=_C.ptr(self.ws[1]), posedirs_packed=_C.ptr(core._packed_posedirs()),
                    posedirs_bwd_packed=_C.ptr(core._packed_posedirs_bwd()), skin_idx=_C.ptr(core.skin_idx), skin_w=_C.ptr(core.skin_w),
                    skin_k=int(core.skin_idx.shape[1]), joint_ptr=_C.ptr(self.jcsr[0]), joint_vidx=_C.ptr(self.jcsr[1]), joint_w=_C.ptr(self.jcsr[2]),
                    extra_vertex_ids=_C.ptr(core.extra_vertex_ids), segment_joints_host=self.segj, num_segments=len(self.names),
                    body_segment=self.segment("body_pose"), num_vertices=core.V, num_joints=core.J, joint_rows=self.rows, **lmk)
