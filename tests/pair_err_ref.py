"""float64 statement of the pose-pair error rule (include/dposer_hip.h, dposer_pose_pair_errors; lib/dataset/AMASS.py:275-316):
from the vertices / joints of oracle.fk_ref.smplx_forward, the per-hypothesis MPVPE over a vertex list, MPJPE over a list of rows of the
LBS joint output (tree joints, vertex-selected extras and barycentric landmarks are all rows of that output), scaled, and the minimum
over the hypotheses."""
import numpy as np

from oracle import fk_ref

PARTS = ("left_leg", "right_leg", "left_arm", "right_arm", "trunk", "hands", "legs", "arms", None)


def part_lists(part):
    """(vert_idx, joint_idx) of a body part as the evaluator builds them (joint index + 1 skips the pelvis); (None, None) for part=None."""
    if part is None:
        return None, None
    from dposer_amd.body_model.utils import BodyPartIndices, BodySegIndices
    return np.array(getattr(BodySegIndices, part)), np.array(getattr(BodyPartIndices, part)) + 1


def bodies(asset, pose_body, betas=None, round_fp32=False):
    """(vertices [N, V, 3], joints [N, J + extras + landmarks, 3]) in float64; ``round_fp32`` rounds both once to fp32 (what a body
    model that hands out fp32 tensors does) before they are widened again."""
    v, j, _, _ = fk_ref.smplx_forward(asset, np.asarray(pose_body, np.float64), betas=None if betas is None else np.asarray(betas, np.float64),
                                      dtype=np.float64)
    if round_fp32:
        v, j = v.astype(np.float32).astype(np.float64), j.astype(np.float32).astype(np.float64)
    return v, j


def pair_errors(asset, ref_pose, hyp_pose, vert_idx=None, joint_idx=None, scale=1.0, betas=None, round_fp32=False):
    """ref_pose [B, 63], hyp_pose [B, H, 63] (or [B, 63]); betas [B, nb] per sample or None.  Returns float64
    {"mpvpe_h", "mpjpe_h"} [B, H] and {"mpvpe", "mpjpe"} [B] (NaN-propagating minimum, as torch.min)."""
    ref_pose, hyp_pose = np.asarray(ref_pose), np.asarray(hyp_pose)
    if hyp_pose.ndim == 2:
        hyp_pose = hyp_pose[:, None]
    B, H = hyp_pose.shape[:2]
    vr, jr = bodies(asset, ref_pose, betas, round_fp32)
    if vert_idx is not None:
        vr = vr[:, np.asarray(vert_idx)]
    if joint_idx is not None:
        jr = jr[:, np.asarray(joint_idx)]
    ev, ej = np.zeros((B, H)), np.zeros((B, H))
    for h in range(H):
        vh, jh = bodies(asset, hyp_pose[:, h], betas, round_fp32)
        if vert_idx is not None:
            vh = vh[:, np.asarray(vert_idx)]
        if joint_idx is not None:
            jh = jh[:, np.asarray(joint_idx)]
        ev[:, h] = np.sqrt(((vh - vr) ** 2).sum(-1)).mean(-1) * scale
        ej[:, h] = np.sqrt(((jh - jr) ** 2).sum(-1)).mean(-1) * scale

    def nanmin(x):
        out = x.min(axis=1)
        out[np.isnan(x).any(axis=1)] = np.nan
        return out
    return {"mpvpe_h": ev, "mpjpe_h": ej, "mpvpe": nanmin(ev), "mpjpe": nanmin(ej)}
