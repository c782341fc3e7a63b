"""Rotation-representation conversions -- counterpart of the rotation part of the reference's
lib/utils/transforms.py (rot6d_to_axis_angle :197-224, rot6d_to_mat3x3 :227-235,
axis_angle_to_rot6d :238-255, axis_angle_to_mat3x3 :258-261).

All four directions are HIP kernels (dposer_rot6d_to_rotmat, dposer_rodrigues, dposer_rotmat_to_axis_angle,
dposer_rot6d_to_axis_angle).  The reference delegates the axis-angle <-> matrix directions to the un-vendored
``torchgeometry``; its published algorithms are restated (torchgeometry is absent and the reference holds no test for them:
parity unpinned against torchgeometry itself, but pinned against ``scipy.spatial.transform.Rotation`` -- an independent
implementation of the same maps -- in tests/test_gpu_fk.py).  ``rigid_transform_3D`` / ``rigid_align`` (:264-286) run as one batched
HIP call (dposer_rigid_align); ``rotate_points`` / ``get_rotation_matrix_x`` / ``get_rotation_matrix_y`` (:289-312) are the host helpers
of ``vis_skeletons``; ``procrustes`` / ``align_to_gt`` (:48-155) have no caller in the reference and are not rebuilt.
"""
import numpy as np
import torch
import torch.nn.functional as F

from .. import _C


def _launch_rot(fn_name, x, in_w):
    _C.require_gpu(x, fn_name + " input")
    x = x.reshape(-1, in_w).contiguous().float()
    out = torch.empty(x.shape[0], 3, 3, dtype=torch.float32, device=x.device)
    if x.shape[0] == 0:
        return out
    _C.check(getattr(_C.lib(), fn_name)(_C.ptr(x), _C.ptr(out), x.shape[0], _C.stream_ptr()), fn_name)
    return out


def rot6d_to_mat3x3(rot6d):
    """[n, 6] (row-major 3x2 = first two columns of R) -> [n, 3, 3] by Gram-Schmidt (transforms.py:227-235)."""
    return _launch_rot("dposer_rot6d_to_rotmat", rot6d, 6)


def batch_rodrigues(rot_vecs):
    """smplx.lbs.batch_rodrigues: [n, 3] axis-angle -> [n, 3, 3]."""
    return _launch_rot("dposer_rodrigues", rot_vecs, 3)


def axis_angle_to_mat3x3(angle_axis):
    """transforms.py:258-261 (tgm.angle_axis_to_rotation_matrix(...)[:, :3, :3]).  torchgeometry switches to a
    first-order Taylor form for theta^2 <= 1e-6; the Rodrigues kernel (angle = ||r + 1e-8||) agrees to fp32
    rounding there."""
    return batch_rodrigues(angle_axis)


def axis_angle_to_rot6d(angle_axis):
    """transforms.py:238-255: first two columns of the rotation matrix, row-major."""
    return axis_angle_to_mat3x3(angle_axis)[:, :3, :2].reshape(-1, 6)


def _launch_to_aa(fn_name, x, in_w):
    _C.require_gpu(x, fn_name + " input")
    x = x.reshape(-1, in_w).contiguous().float()
    out = torch.empty(x.shape[0], 3, dtype=torch.float32, device=x.device)
    if x.shape[0]:
        _C.check(getattr(_C.lib(), fn_name)(_C.ptr(x), _C.ptr(out), x.shape[0], _C.stream_ptr()), fn_name)
    return out


def rotmat_to_axis_angle(R):
    """Rotation matrix [n,3,3] -> axis-angle [n,3] through the unit quaternion (the route
    torchgeometry.rotation_matrix_to_angle_axis takes: matrix -> quaternion -> angle-axis); one HIP kernel."""
    return _launch_to_aa("dposer_rotmat_to_axis_angle", R, 9)


def rot6d_to_axis_angle(rot6d):
    """transforms.py:197-224 (Gram-Schmidt + matrix -> axis-angle + NaN -> 0) in one HIP kernel."""
    return _launch_to_aa("dposer_rot6d_to_axis_angle", rot6d, 6)


def cam_crop2full(crop_cam, center, scale, full_img_shape, focal_length):
    """Weak-perspective crop camera (s, tx, ty) [N, 3] -> full-image translation (tx, ty, tz) [N, 3] (transforms.py:172-190).
    ``center`` [N, 2] bbox centre, ``scale`` [N] bbox size / 200, ``full_img_shape`` [N, 2] (height, width), ``focal_length`` [N]
    or scalar.  Host-side helper of run/fitting.py: builds SMPLify's ``init_cam_t``."""
    img_h, img_w = full_img_shape[:, 0], full_img_shape[:, 1]
    bs = scale * 200 * crop_cam[:, 0] + 1e-9
    tz = 2 * focal_length / bs
    tx = 2 * (center[:, 0] - img_w / 2.) / bs + crop_cam[:, 1]
    ty = 2 * (center[:, 1] - img_h / 2.) / bs + crop_cam[:, 2]
    return torch.stack([tx, ty, tz], dim=-1)


def estimate_focal_length(img_h, img_w):
    """Focal length of a ~55 degree field of view: the image diagonal (transforms.py:193-194)."""
    return (img_w * img_w + img_h * img_h) ** 0.5


def rigid_align_device(src, dst, transform=True, aligned=True, mean_dist=True):
    """dposer_rigid_align on device tensors ``src``, ``dst`` [B, N, 3]: (transform [B, 13] = (c, R row-major, t), aligned [B, N, 3],
    mean_dist [B]), None for the outputs not asked for.  One launch, no allocation inside the call, no host synchronisation."""
    _C.require_gpu(src, "rigid_align src")
    _C.require_gpu(dst, "rigid_align dst")
    if src.dim() != 3 or src.shape[-1] != 3 or src.shape != dst.shape or src.shape[1] < 1:
        raise ValueError(f"rigid_align: point sets must both be [B, N, 3] with N >= 1, got {tuple(src.shape)} and {tuple(dst.shape)}")
    src, dst = src.contiguous().float(), dst.contiguous().float()
    B, N = src.shape[0], src.shape[1]
    T = torch.empty(B, 13, dtype=torch.float32, device=src.device) if transform else None
    out = torch.empty_like(src) if aligned else None
    md = torch.empty(B, dtype=torch.float32, device=src.device) if mean_dist else None
    if B:
        args = _C.RigidAlignArgs(src.data_ptr(), dst.data_ptr(), B, N, T.data_ptr() if transform else None,
                                 out.data_ptr() if aligned else None, md.data_ptr() if mean_dist else None)
        _C.check(_C.lib().dposer_rigid_align(args, _C.stream_ptr()), "dposer_rigid_align")
    return T, out, md


def _as_device_pairs(A, B):
    """(A, B) as device tensors [B, N, 3] + how to hand results back: host arrays are moved to the GPU (there is no CPU arithmetic path)."""
    is_np = not torch.is_tensor(A)
    if is_np:
        np_dtype = np.float64 if np.asarray(A).dtype == np.float64 else np.float32
        A = torch.as_tensor(np.ascontiguousarray(A, dtype=np.float32), device="cuda")
        B = torch.as_tensor(np.ascontiguousarray(np.asarray(B), dtype=np.float32), device="cuda")
    else:
        np_dtype = None
        B = torch.as_tensor(B, device=A.device)
    single = A.dim() == 2
    if single:
        A, B = A[None], B[None]
    back = (lambda x: x.cpu().numpy().astype(np_dtype)) if is_np else (lambda x: x)
    return A, B, single, back


def rigid_transform_3D(A, B):
    """transforms.py:264-280: the similarity (c, R, t) taking the points A onto B, for one pair [N, 3] or a batch [B, N, 3] (then c [B],
    R [B, 3, 3], t [B, 3]).  numpy in -> numpy out; device tensor in -> device tensors out, without a synchronisation."""
    A, B, single, back = _as_device_pairs(A, B)
    T, _, _ = rigid_align_device(A, B, aligned=False, mean_dist=False)
    c, R, t = T[:, 0], T[:, 1:10].reshape(-1, 3, 3), T[:, 10:13]
    if single:
        c, R, t = c[0], R[0], t[0]
    return back(c), back(R), back(t)


def rigid_align(A, B):
    """transforms.py:283-286: A under the similarity that takes it onto B, [N, 3] or [B, N, 3]; numpy or device tensors as above."""
    A, B, single, back = _as_device_pairs(A, B)
    _, out, _ = rigid_align_device(A, B, transform=False, mean_dist=False)
    return back(out[0] if single else out)


def rotate_points(points, rotation_matrix):
    """transforms.py:289-290: ``points [..., 3]`` under ``rotation_matrix`` (host helper of ``vis_skeletons``)."""
    return np.dot(points, rotation_matrix.T)


def get_rotation_matrix_x(angle):
    """transforms.py:293-301: rotation about the x axis."""
    return np.array([[1, 0, 0], [0, np.cos(angle), -np.sin(angle)], [0, np.sin(angle), np.cos(angle)]])


def get_rotation_matrix_y(angle):
    """transforms.py:304-312: rotation about the y axis."""
    return np.array([[np.cos(angle), 0, np.sin(angle)], [0, 1, 0], [-np.sin(angle), 0, np.cos(angle)]])
