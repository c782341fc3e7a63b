"""SMPLify's fitting losses -- counterpart of the reference's lib/body_model/fitting_losses.py.

Plain torch: the step-by-step path of ``tasks.smplify.SMPLify(fused=False)`` differentiates these with autograd, and they are the
readable statement of what the one-call loop's kernels (``dposer_smplify_optimize``, csrc/smplify.hip) compute.
"""
import torch

from . import constants


def perspective_projection(points, rotation, translation, focal_length, camera_center):
    """Pinhole projection of ``points`` [B, N, 3] -> [B, N, 2] (fitting_losses.py:6-38).
    ``focal_length`` [B] or scalar, ``camera_center`` [B, 2].  ``translation`` is NOT applied (the reference never reads it): the
    callers put the camera translation into the body model as ``transl``."""
    B = points.shape[0]
    K = torch.zeros([B, 3, 3], device=points.device)
    K[:, 0, 0] = focal_length
    K[:, 1, 1] = focal_length
    K[:, 2, 2] = 1.
    K[:, :-1, -1] = camera_center
    points = torch.einsum("bij,bkj->bki", rotation, points)
    projected = points / points[:, :, -1].unsqueeze(-1)
    projected = torch.einsum("bij,bkj->bki", K, projected)
    return projected[:, :, :-1]


def gmof(x, sigma):
    """Geman-McClure robust error s^2 x^2 / (s^2 + x^2) (fitting_losses.py:41-47)."""
    x_squared = x ** 2
    sigma_squared = sigma ** 2
    return (sigma_squared * x_squared) / (sigma_squared + x_squared)


def angle_prior(pose):
    """exp(+-theta)^2 penalty on the knee / elbow bends, body-pose entries 52, 55, 9, 12 (fitting_losses.py:48-54; the indices are the
    full-pose ones minus the 3 global-orientation entries)."""
    signs = torch.tensor([1., -1., -1, -1.], device=pose.device)
    return torch.exp(pose[:, [55 - 3, 58 - 3, 12 - 3, 15 - 3]] * signs) ** 2


def body_fitting_loss(body_pose, betas, model_joints, camera_t, camera_center, joints_2d, joints_conf, pose_prior, quan_t,
                      focal_length=5000, sigma=100, pose_prior_weight=4.78, shape_prior_weight=5, angle_prior_weight=15.2,
                      output="mean", verbose=True):
    """fitting_losses.py:57-105: per image conf^2-weighted GMoF reprojection + w_pose^2 prior + w_angle^2 angle prior + w_shape^2 |betas|^2.
    The prior is a scalar (``pose_prior(body_pose, betas, quan_t)``: sum / batch_size) broadcast over the batch.
    ``output``: 'mean' (over the batch), 'sum', or 'reprojection' ([B, n_joints], before the sum over joints)."""
    B = body_pose.shape[0]
    rotation = torch.eye(3, device=body_pose.device).unsqueeze(0).expand(B, -1, -1)
    projected = perspective_projection(model_joints, rotation, camera_t, focal_length, camera_center)
    reprojection_error = gmof(projected - joints_2d, sigma)
    reprojection_loss = (joints_conf ** 2) * reprojection_error.sum(dim=-1)
    pose_prior_loss = (pose_prior_weight ** 2) * pose_prior(body_pose, betas, quan_t) if pose_prior is not None else 0.0
    angle_prior_loss = (angle_prior_weight ** 2) * angle_prior(body_pose).sum(dim=-1)
    shape_prior_loss = (shape_prior_weight ** 2) * (betas ** 2).sum(dim=-1)
    total_loss = reprojection_loss.sum(dim=-1) + pose_prior_loss + angle_prior_loss + shape_prior_loss
    if verbose:
        print(f"Reprojection Loss: {reprojection_loss.sum(dim=-1).mean().item():.2f}")
        print(f"Angle Prior Loss: {angle_prior_loss.mean().item():.2f}")
        print(f"Shape Prior Loss: {shape_prior_loss.mean().item():.2f}")
        if pose_prior is not None:
            print(f"Pose Prior Loss: {pose_prior_loss.mean().item():.2f}")
    if output == "sum":
        return total_loss.sum()
    if output == "reprojection":
        return reprojection_loss
    return total_loss.mean()


def camera_fitting_loss(model_joints, camera_t, camera_t_est, camera_center, joints_2d, joints_conf, focal_length=5000, depth_loss_weight=100):
    """fitting_losses.py:108-131: squared reprojection error of the OpenPose hips / shoulders -- or, for an image where any of those four
    confidences is not > 0, of the ground-truth hips / shoulders -- plus depth_loss_weight^2 (t_z - t_z_est)^2; SUM over the batch."""
    B = model_joints.shape[0]
    rotation = torch.eye(3, device=model_joints.device).unsqueeze(0).expand(B, -1, -1)
    projected = perspective_projection(model_joints, rotation, camera_t, focal_length, camera_center)
    op_ind = [constants.JOINT_IDS[j] for j in ("OP RHip", "OP LHip", "OP RShoulder", "OP LShoulder")]
    gt_ind = [constants.JOINT_IDS[j] for j in ("Right Hip", "Left Hip", "Right Shoulder", "Left Shoulder")]
    err_op = (joints_2d[:, op_ind] - projected[:, op_ind]) ** 2
    err_gt = (joints_2d[:, gt_ind] - projected[:, gt_ind]) ** 2
    is_valid = (joints_conf[:, op_ind].min(dim=-1)[0][:, None, None] > 0).float()
    reprojection_loss = (is_valid * err_op + (1 - is_valid) * err_gt).sum(dim=(1, 2))
    depth_loss = (depth_loss_weight ** 2) * (camera_t[:, 2] - camera_t_est[:, 2]) ** 2
    return (reprojection_loss + depth_loss).sum()
