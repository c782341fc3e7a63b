"""Human-mesh recovery from 2D keypoints and its EHF evaluation -- what the reference's run/fitting.py:46-149 does per image, for B
images at a time: box -> initial camera (cam_crop2full) -> ONE SMPLify call -> one body-model forward -> ONE dposer_ehf_eval ->
one render_meshes call per image size with the photos as backgrounds.  cv2 is never imported: photos are arrays (PIL decodes the JPEGs of
``run_folder`` when it is importable), overlays are written by body_model.visual.write_image."""
import glob
import json
import os
import warnings

import numpy as np
import torch

from ..body_model import constants
from ..body_model.visual import render_meshes, renderer_lights, write_image
from ..utils.preprocess import compute_bbox
from ..utils.transforms import cam_crop2full, estimate_focal_length

N_POSES = 22                                   # root orientation + 21 body joints (fitting.py:53)
EHF_BOX = (0, 400, 100, 1000, 1200)            # fitting.py:72: the fixed box [image index, min_x, min_y, max_x, max_y] of the EHF photos
EHF_BEND_MIN_Y = 400                           # fitting.py:71: a keypoint box starting below this row starts from the bend pose
MESH_COLOR = (0.4, 0.6, 0.93)                  # Renderer(same_mesh_color=True)


def initial_fit(smpl, keypoints25, image_shapes, boxes=None, crop_cam=(0.9, 0, 0), init_pose=None):
    """The inputs of SMPLify for B images (fitting.py:79-108): ``keypoints25`` [B, 25, 3] OpenPose (x, y, confidence), ``image_shapes``
    [B, 2] (height, width), ``boxes`` [B, 4] or [B, 5] ([image index,] min_x, min_y, max_x, max_y; None: the EHF box for every image),
    ``init_pose`` [B, 66] or [66] (None: the mean pose).  Returns a dict of device tensors: focal_length [B], camera_center [B, 2],
    init_cam_t [B, 3], keypoints [B, 49, 3], init_pose [B, 66], init_betas [B, 10], center [B, 2], scale [B]."""
    dev = smpl.mean_poses.device
    shapes = np.asarray(image_shapes, dtype=np.int64).reshape(-1, 2)
    B = shapes.shape[0]
    box = np.tile(np.asarray(EHF_BOX[1:], np.float64), (B, 1)) if boxes is None else np.asarray(boxes, np.float64)[:, -4:]
    # bbox_from_detector (rescale 1.1) and estimate_focal_length in the host's fp64, as the dataset's __getitem__ forms them
    center = torch.tensor(np.stack([(box[:, 0] + box[:, 2]) / 2.0, (box[:, 1] + box[:, 3]) / 2.0], 1), device=dev).float()
    size = np.maximum((box[:, 2] - box[:, 0]) * constants.CROP_ASPECT_RATIO, box[:, 3] - box[:, 1])
    scale = torch.tensor(size / 200.0 * 1.1, device=dev).float()
    focal = torch.tensor([estimate_focal_length(int(h), int(w)) for h, w in shapes], dtype=torch.float64, device=dev).float()
    img_h = torch.tensor(shapes[:, 0], device=dev).float()
    img_w = torch.tensor(shapes[:, 1], device=dev).float()
    full_img_shape = torch.stack((img_h, img_w), dim=-1)
    pred_cam_crop = torch.tensor([list(crop_cam)], dtype=torch.float32, device=dev).repeat(B, 1)
    init_cam_t = cam_crop2full(pred_cam_crop, center, scale, full_img_shape, focal)
    kp = torch.zeros(B, 49, 3, dtype=torch.float64, device=dev)
    kp[:, :25] = torch.as_tensor(np.asarray(keypoints25, np.float64).reshape(B, 25, 3), device=dev)
    if init_pose is None:
        pose = smpl.mean_poses[:N_POSES * 3].unsqueeze(0).repeat(B, 1)
    else:
        pose = torch.as_tensor(init_pose, dtype=torch.float32, device=dev).reshape(-1, N_POSES * 3).expand(B, -1).contiguous()
    betas = smpl.mean_shape.unsqueeze(0).repeat(B, 1)
    return dict(focal_length=focal, camera_center=torch.stack((img_w, img_h), dim=-1) / 2, init_cam_t=init_cam_t, keypoints=kp,
                init_pose=pose, init_betas=betas, center=center, scale=scale)


def render_overlays(vertices, faces, focal_length, image_shapes, images):
    """Renderer.render_front_view (visual.py) for every image at once: mesh b over photo b (uint8 RGB [H, W, 3]), one render_meshes call
    per image size.  Returns (overlays: list of uint8 device tensors [H, W, 3], depth: list of fp32 [H, W])."""
    dev = vertices.device
    shapes = [tuple(int(x) for x in s) for s in np.asarray(image_shapes).reshape(-1, 2)]
    overlays, depths = [None] * len(shapes), [None] * len(shapes)
    for hw in sorted(set(shapes)):
        idx = [i for i, s in enumerate(shapes) if s == hw]
        sel = torch.tensor(idx, device=dev)
        fl = focal_length[sel].float()
        K = torch.stack([fl, fl, torch.full_like(fl, float(hw[1] // 2)), torch.full_like(fl, float(hw[0] // 2))], dim=1)
        bg = torch.stack([torch.as_tensor(np.ascontiguousarray(images[i]), dtype=torch.uint8, device=dev) for i in idx])
        out = render_meshes(vertices[sel].contiguous(), faces, K, hw, base_color=torch.tensor(MESH_COLOR, device=dev), lights=renderer_lights(),
                            ambient=0.0, smooth=True, background=bg, outputs=("rgb", "depth"))
        for k, i in enumerate(idx):
            overlays[i], depths[i] = out["rgb"][k], out["depth"][k]
    return overlays, depths


def fit_and_evaluate(smplify, mocap, keypoints25, image_shapes, gt_vertices=None, boxes=None, crop_cam=(0.9, 0, 0), init_pose=None,
                     images=None, outdir=None, names=None, **smplify_kwargs):
    """Fit B images in one SMPLify call and evaluate them in one dposer_ehf_eval call.  ``smplify``: a tasks.smplify.SMPLify (its
    ``focal_length`` is set to the per-image estimates, as fitting.py:117 builds it); ``mocap``: a dataset.mocap_dataset.MocapDataset (the
    evaluation's body model and regressor); ``gt_vertices`` [B, V, 3] (None: no evaluation); ``images`` (uint8 RGB arrays) with
    ``outdir``: the overlays are written as ``<name>_mesh_fit.png``.  Returns a dict of device tensors: pose, betas, camera_translation,
    reprojection_loss, vertices, and pa_mpjpe_body / mpjpe_body [B], overlays / depth (lists) when asked for."""
    init = initial_fit(smplify.smpl, keypoints25, image_shapes, boxes, crop_cam, init_pose)
    smplify.focal_length = init["focal_length"]
    results = smplify(init["init_pose"].detach(), init["init_betas"].detach(), init["init_cam_t"].detach(), init["camera_center"],
                      init["keypoints"], **smplify_kwargs)
    pose, betas, cam_t, reproj = results
    with torch.no_grad():
        vertices = smplify.smpl(betas=betas, body_pose=pose[:, 3:], global_orient=pose[:, :3], pose2rot=True, transl=cam_t).vertices
    out = dict(pose=pose, betas=betas, camera_translation=cam_t, reprojection_loss=reproj, vertices=vertices, init=init)
    if gt_vertices is not None:
        out.update(mocap.eval_EHF_batch(results, gt_vertices))
    if images is not None:
        out["overlays"], out["depth"] = render_overlays(vertices, smplify.smpl.faces, init["focal_length"], image_shapes, images)
        if outdir is not None:
            os.makedirs(outdir, exist_ok=True)
            for k, img in enumerate(out["overlays"]):
                name = names[k] if names is not None else f"{k:06d}"
                write_image(os.path.join(outdir, f"{name}_mesh_fit.png"), img.cpu().numpy())
    return out


def _read_rgb(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"))


def run_folder(data_dir, outdir, smplify, mocap, batch_size=32, image_shapes=None, fixed_box=EHF_BOX, bend_min_y=EHF_BEND_MIN_Y,
               bend_pose_path=constants.BEND_POSE_PATH, **smplify_kwargs):
    """run/fitting.py over a folder of ``*_img.jpg`` / ``*_2Djnt.json`` / ``*_align.ply`` triples, ``batch_size`` images per SMPLify
    call.  ``fixed_box`` / ``bend_min_y`` / ``bend_pose_path``: the script's EHF constants (a keypoint box whose min_y exceeds
    ``bend_min_y`` starts from the bend pose; ``fixed_box=None`` uses the keypoint boxes).  Without PIL the photos cannot be decoded:
    pass ``image_shapes`` [(h, w)] and no overlays are written.  Prints and returns the per-image metrics."""
    from ..utils.preprocess import load_ply
    img_paths = sorted(glob.glob(f"{data_dir}/*_img.jpg"))
    json_paths = sorted(glob.glob(f"{data_dir}/*_2Djnt.json"))
    ply_paths = sorted(glob.glob(f"{data_dir}/*_align.ply"))
    try:
        import PIL  # noqa: F401
        have_pil = True
    except ImportError:
        have_pil = False
    if not have_pil and image_shapes is None:
        raise RuntimeError("decoding the photos needs PIL; without it pass image_shapes=[(h, w), ...] (no overlays are written)")
    n = len(json_paths)
    stem = lambda p, tail: os.path.basename(p)[:-len(tail)]
    if len(ply_paths) != n or [stem(p, "_2Djnt.json") for p in json_paths] != [stem(p, "_align.ply") for p in ply_paths] or (
            image_shapes is None and [stem(p, "_img.jpg") for p in img_paths] != [stem(p, "_2Djnt.json") for p in json_paths]) or (
            image_shapes is not None and len(image_shapes) != n):
        raise ValueError(f"{data_dir}: the *_img.jpg / *_2Djnt.json / *_align.ply files (or image_shapes) do not pair up one to one")
    dev = smplify.smpl.mean_poses.device
    bend_pose = None
    if os.path.exists(bend_pose_path):
        bend_pose = np.load(bend_pose_path)["pose"].reshape(-1)[:N_POSES * 3].astype(np.float32)
    all_results = {"pa_mpjpe_body": [], "mpjpe_body": []}
    for lo in range(0, n, batch_size):
        hi = min(n, lo + batch_size)
        kps, boxes, bends = [], [], []
        for jp in json_paths[lo:hi]:
            with open(jp) as fh:
                data = json.load(fh)
            kps.append(np.array(data["people"][0]["pose_keypoints_2d"]).reshape(25, 3))
            kbox = compute_bbox(data)
            if kbox.ndim != 2:
                raise ValueError(f"{jp}: no person with a visible keypoint")
            bends.append(bool(kbox[0, 2] > bend_min_y))
            boxes.append(np.asarray(fixed_box if fixed_box is not None else kbox[0], np.float64))
        images = [_read_rgb(p) for p in img_paths[lo:hi]] if have_pil and image_shapes is None else None
        shapes = [im.shape[:2] for im in images] if images is not None else list(image_shapes[lo:hi])
        init_pose = None
        if any(bends):
            if bend_pose is None:
                warnings.warn(f"{bend_pose_path} not found: starting from the mean pose where the script starts from the bend pose")
            else:
                mean = smplify.smpl.mean_poses[:N_POSES * 3].cpu().numpy()
                init_pose = np.stack([bend_pose if b else mean for b in bends])
        gt = torch.as_tensor(np.stack([np.asarray(load_ply(p), np.float32) for p in ply_paths[lo:hi]]), device=dev)
        names = [os.path.splitext(os.path.basename(p))[0] for p in img_paths[lo:hi]] if len(img_paths) == n else None
        res = fit_and_evaluate(smplify, mocap, np.stack(kps), shapes, gt, np.stack(boxes), init_pose=init_pose, images=images, outdir=outdir,
                               names=names, **smplify_kwargs)
        for k in all_results:
            all_results[k].extend(res[k].cpu().tolist())
    print("results on whole dataset:")
    mocap.print_eval_result(all_results)
    return all_results
