"""The generation-process videos -- library form of the ``generation_process`` task of the reference's run/demo.py:164-209: a sampler
trajectory rendered as bodies, one video per sample.

The reference keeps all 1000 states of the predictor-corrector sampler, takes every 10th (``trajs[9::10]``), and then renders and encodes
one frame at a time.  Here the sampler stores only every 10th state (``traj_stride=10``: the same states), and the frames of every video
go through one body-model forward, one ``render_meshes`` call and ``utils.motion_video.write_video`` (30 fps, uncompressed AVI: a
``.mp4`` name gets the ``.avi`` suffix)."""
import os

import torch

from ..algorithms.advanced import sampling
from ..body_model import visual
from ..utils.motion_video import write_video

CANVAS = (512, 384)                   # run/demo.py's bg_img, focal and princpt
FOCAL = (1500, 1500)
PRINCPT = (200, 192)
STRIDE = 10                           # trajs[9::10]
FPS = 30


def generation_process(model, sde, config, normalizer, body_model, target_path, video_num=3, *, sampling_eps=1e-3, inverse_scaler=None,
                       pose_dim=None, device=None, seed=None, name="generation_process{}.mp4"):
    """demo.py:164-209.  ``config.sampling.method`` must be 'pc' or 'dpm' (the ODE sampler keeps no trajectory).  Writes ``video_num``
    videos of ``sde.N // 10`` frames ('dpm': one frame per solver step) into ``target_path`` and returns their paths."""
    os.makedirs(target_path, exist_ok=True)
    method = str(config.sampling.method).lower()
    assert method in ("pc", "dpm")                      # we don't save trajectories for ode sampler
    dev = torch.device(device) if device is not None else next(model.parameters()).device
    D = int(pose_dim) if pose_dim is not None else int(model.n_poses * model.joint_dim)
    fn = sampling.get_sampling_fn(config, sde, (video_num, D), inverse_scaler or (lambda v: v), sampling_eps, device=dev)
    kw = {} if seed is None else {"seed": seed}
    # 'pc': [N // 10, video_num, D] == trajs[9::10];  'dpm': the few-step solver has config.sampling.dpm_steps states, all kept
    trajs, _ = fn(model, observation=None, traj_stride=STRIDE if method == "pc" else 1, **kw)
    num_frame = int(trajs.shape[0])
    with torch.no_grad():
        poses = normalizer.offline_denormalize(trajs.transpose(0, 1).reshape(video_num * num_frame, D), to_axis=True)
        body_out = body_model(pose_body=poses)
        H, W = CANVAS
        rgb, mask = visual._render_mesh_batch(body_out.v, body_out.f, H, W, FOCAL, PRINCPT, ["front"] * len(poses), body_out.v.device)
        frames = torch.where(mask[..., None], rgb, torch.full_like(rgb, 255)).reshape(video_num, num_frame, H, W, 3)
    paths = []
    for idx in range(video_num):
        path = write_video(os.path.join(target_path, name.format(idx)), frames[idx], FPS)
        print(f"Video saved at {path}")
        paths.append(path)
    return paths
