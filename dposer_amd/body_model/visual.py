"""lib/body_model/visual.py: the mesh renderer behind every user-facing entry point of the reference (``render_mesh``,
``multiple_render``, ``faster_render``, ``Renderer``, ``save_obj``), on the package's own rasteriser (csrc/render.hip,
``dposer_render_meshes``; rules in include/dposer_hip.h).  The reference renders one mesh at a time through pyrender (OpenGL) or
pytorch3d; here B meshes go through one call.

Shading is Lambert plus ambient, ``c = clamp(base * (ambient + sum_l I_l max(0, n . l)), 0, 1)``, with no specular term.  pyrender's
physically based shader divides its Lambert term by pi and adds a specular lobe; the presets below take pyrender's light intensities
divided by pi (and pytorch3d's Phong weights for ``faster_render``), so the images read like the reference's.  Parity with pyrender or
pytorch3d is not pinned.  Images are written as true RGB (the reference's ``render_mesh`` route hands RGB arrays to ``cv2.imwrite``,
which expects BGR, so its saved bodies are channel-swapped).

Skeleton plots (``vis_skeletons``, ``visualize_skeleton_sequence``, ``visualize_3d_skeleton``; visual.py:18-119, one matplotlib 3-D figure
per frame there) go through ``draw_skeletons``: every frame of a sequence in one ``dposer_draw_skeletons`` call (csrc/draw.hip).  The rules,
in full in include/dposer_hip.h:

* view: orthographic, an upright front view of the joints handed to ``vis_skeletons`` (its flip by pi about x followed by matplotlib's
  ``plot(x, z, -y)`` at ``view_init(0, -90)``): x to the right, y up, a larger z nearer;
* frames are 640 x 480 on white, as ``plt.savefig`` makes them; a sequence shares one scale and one centre (min / max over all frames,
  padding ratio 1.2, the largest padded extent of the three axes spans min(H, W), the x / y centre of the bounds lands on the image
  centre); a single frame uses its own bounds; ``ax_lims`` (x, y, z bounds already padded) is honoured the same way;
* bones are segments ``LINE_WIDTH_PX`` wide (matplotlib's linewidth 2 pt at 100 dpi), joints discs of radius ``JOINT_RADIUS_PX`` (its
  default 6 pt marker); coverage is ``clamp(r + 0.5 - distance, 0, 1)`` at pixel centres;
* painter's order per frame, one depth per primitive (a bone: the mean of its ends; a disc: its joint, 1e-3 nearer), far to near;
* colours are what the reference plots: matplotlib's ``rainbow`` at ``linspace(0, 1, K + 2)`` with red and blue swapped (visual.py:35),
  frozen in ``SKELETON_COLORS_21`` for the SMPL bone list; a joint's disc takes the colour of the last bone that touches it.

Pixel parity with matplotlib is not a goal and is not claimed (no axes box perspective, no figure margins, no title text: ``title`` is
accepted and ignored).  A ``.mp4`` path produces an uncompressed ``.avi`` beside it (``utils.motion_video.write_video``)."""
import colorsys
import ctypes as C
import math
import os
import random
import struct
import zlib

import numpy as np
import torch

_KEY_IDS = (1 << 32) - 2            # b * F + f must stay below 2^32 - 1; list offsets: 5 entries per face at most
_MAX_ENTRIES = (1 << 32) - 1

# presets (see the module docstring)
RENDER_MESH_COLOR = (0.93, 0.6, 0.4)
RENDER_MESH_AMBIENT = 0.3
RENDER_MESH_LIGHT = 0.8 / math.pi
FASTER_SIZE = 256
FASTER_FOV_DEG = 60.0
FASTER_AMBIENT = 0.5                 # pytorch3d PointLights: ambient 0.5, diffuse 0.3 (materials: 1.0)
FASTER_LIGHT = 0.3
RENDERER_LIGHT = 3.0 / math.pi


def _dev():
    return torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")


def _vf_csr(faces, V):
    """vertex -> face CSR of a face list: (ptr int32 [V + 1], face int32 [3F]).  The faces of a vertex are ordered by their sorted vertex
    indices, not by their position in the list, so the smooth normals do not change with the face order (a sort, no atomics)."""
    F = faces.shape[0]
    vid = faces.reshape(-1).long()
    fid = torch.arange(F, device=faces.device, dtype=torch.int64).repeat_interleave(3)
    srt = torch.sort(faces.long(), dim=1).values
    order = torch.arange(3 * F, device=faces.device)
    for key in (srt[:, 2][fid], srt[:, 1][fid], srt[:, 0][fid], vid):           # least significant key first, stable passes
        order = order[torch.sort(key[order], stable=True).indices]
    ptr = torch.zeros(V + 1, dtype=torch.int64, device=faces.device)
    ptr[1:] = torch.cumsum(torch.bincount(vid, minlength=V), 0)
    return ptr.to(torch.int32).contiguous(), fid[order].to(torch.int32).contiguous()


def _as_f32(x, dev, name, shape_tail):
    t = torch.as_tensor(x, dtype=torch.float32, device=dev) if not torch.is_tensor(x) else x.detach()
    if t.device != dev:
        raise ValueError(f"{name} lives on {t.device}, vertices on {dev}")
    t = t.to(torch.float32)
    if tuple(t.shape[-len(shape_tail):]) != shape_tail:
        raise ValueError(f"{name} must end in {shape_tail}, got {tuple(t.shape)}")
    return t


def render_meshes(vertices, faces, intrinsics, image_size, transforms=None, image_of_mesh=None, base_color=(1.0, 1.0, 1.0), lights=(),
                  ambient=(0.0, 0.0, 0.0), smooth=False, background=None, background_color=(0, 0, 0), znear=0.01, zfar=1e4,
                  outputs=("rgb", "depth", "face_id", "mesh_id")):
    """Render ``vertices [B, V, 3]`` (one shared ``faces [F, 3]``) into ``num_images`` images of ``image_size = (H, W)``.

    ``intrinsics [num_images, 4]`` (fx, fy, cx, cy; OpenCV camera: x right, y down, z forward); ``transforms [B, 3, 4]`` model -> camera
    (None: identity); ``image_of_mesh [B]`` (None: mesh b -> image b; meshes of one image are depth-tested together);
    ``base_color [B, 3]`` or ``[3]``; ``lights``: rows (kind, x, y, z, r, g, b), kind 0 directional (toward the light) or 1 point;
    ``background`` uint8 ``[H, W, 3]`` (shared) or ``[num_images, H, W, 3]``, else ``background_color`` (uint8 RGB).
    Returns a dict of device tensors: ``rgb`` uint8 [N, H, W, 3], ``depth`` fp32 [N, H, W] (0 where empty), ``face_id`` / ``mesh_id`` int32
    (-1 where empty), those named in ``outputs``.  ROCm tensors only; no CPU fallback."""
    from .. import _C
    if not torch.is_tensor(vertices):
        raise ValueError("vertices must be a torch tensor on the GPU")
    _C.require_gpu(vertices, "vertices")
    if not torch.is_tensor(faces):
        faces = torch.as_tensor(np.asarray(faces), device=vertices.device)
    _C.require_gpu(faces, "faces")
    dev = vertices.device
    if vertices.dim() != 3 or vertices.shape[-1] != 3:
        raise ValueError(f"vertices must be [B, V, 3], got {tuple(vertices.shape)}")
    if faces.dim() != 2 or faces.shape[-1] != 3:
        raise ValueError(f"faces must be [F, 3], got {tuple(faces.shape)}")
    if faces.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"faces must hold int32 or int64 vertex indices, got {faces.dtype}")
    B, V, F = int(vertices.shape[0]), int(vertices.shape[1]), int(faces.shape[0])
    if B == 0:
        raise ValueError("empty batch: nothing to render")
    if V == 0 or F == 0:
        raise ValueError("a mesh needs vertices and faces")
    if V >= 2 ** 31 or F >= 2 ** 31:
        raise ValueError("meshes of 2^31 vertices or faces and more are not supported")
    H, W = (int(s) for s in image_size)
    if H < 1 or W < 1:
        raise ValueError(f"image_size must be >= 1 in both axes, got {(H, W)}")
    lo, hi = int(faces.min()), int(faces.max())
    if lo < 0 or hi >= V:
        raise ValueError(f"face indices must lie in [0, {V}), got [{lo}, {hi}]")
    unknown = set(outputs) - {"rgb", "depth", "face_id", "mesh_id"}
    if unknown:
        raise ValueError(f"unknown outputs {sorted(unknown)}")

    K = _as_f32(intrinsics, dev, "intrinsics", (4,))
    if K.dim() == 1:
        K = K[None]
    if image_of_mesh is None:
        N = B
        img = None
        if K.shape[0] not in (1, N):
            raise ValueError(f"intrinsics must be [num_images = {N}, 4], got {tuple(K.shape)}")
    else:
        img = torch.as_tensor(image_of_mesh, device=dev).to(torch.int64)
        if img.shape != (B,):
            raise ValueError(f"image_of_mesh must be [B = {B}], got {tuple(img.shape)}")
        N = int(img.max()) + 1 if K.shape[0] == 1 else int(K.shape[0])
        if int(img.min()) < 0 or int(img.max()) >= N:
            raise ValueError(f"image_of_mesh must lie in [0, {N})")
    K = K.expand(N, 4).contiguous() if K.shape[0] == 1 else K.contiguous()
    if K.shape[0] != N:
        raise ValueError(f"intrinsics must be [num_images = {N}, 4], got {tuple(K.shape)}")
    T = (torch.eye(3, 4, device=dev).expand(B, 3, 4) if transforms is None else _as_f32(transforms, dev, "transforms", (3, 4)))
    T = T.expand(B, 3, 4).contiguous()
    col = _as_f32(base_color, dev, "base_color", (3,)).expand(B, 3).contiguous()
    L = torch.as_tensor(np.asarray(lights, dtype=np.float32).reshape(-1, 7), device=dev) if not torch.is_tensor(lights) else lights.to(dev, torch.float32)
    if L.dim() != 2 or L.shape[1] != 7:
        raise ValueError(f"lights must be [L, 7], got {tuple(L.shape)}")
    L = L.contiguous()
    bg, bg_stride = None, 0
    if background is not None:
        bg = torch.as_tensor(background, device=dev) if not torch.is_tensor(background) else background.to(dev)
        if bg.dtype != torch.uint8 or tuple(bg.shape[-3:]) != (H, W, 3) or bg.dim() not in (3, 4) or (bg.dim() == 4 and bg.shape[0] != N):
            raise ValueError(f"background must be uint8 [H, W, 3] or [num_images, H, W, 3], got {bg.dtype} {tuple(bg.shape)}")
        bg = bg.contiguous()
        bg_stride = H * W * 3 if bg.dim() == 4 else 0
    amb = [float(a) for a in np.broadcast_to(np.asarray(ambient, dtype=np.float64), (3,))]
    bgc = [int(c) for c in np.broadcast_to(np.asarray(background_color), (3,))] + [0]

    v = vertices.detach().to(torch.float32).contiguous()
    f32 = faces.to(torch.int32).contiguous()                                         # (int64 faces: converted once)
    vf_ptr, vf_face = _vf_csr(f32, V) if smooth else (None, None)
    out = {}
    if "rgb" in outputs:
        out["rgb"] = torch.empty((N, H, W, 3), dtype=torch.uint8, device=dev)
    if "depth" in outputs:
        out["depth"] = torch.empty((N, H, W), dtype=torch.float32, device=dev)
    if "face_id" in outputs:
        out["face_id"] = torch.empty((N, H, W), dtype=torch.int32, device=dev)
    if "mesh_id" in outputs:
        out["mesh_id"] = torch.empty((N, H, W), dtype=torch.int32, device=dev)

    # calls: groups of whole images whose meshes keep (mesh, face) ids and list offsets in 32 bits
    per_call = min(_KEY_IDS // F, _MAX_ENTRIES // (5 * F))
    if per_call < 1:
        raise ValueError(f"{F} faces per mesh is too many for one call")
    if img is None:
        groups = [(i0, min(N, i0 + per_call), None) for i0 in range(0, N, per_call)]
    else:
        counts = torch.bincount(img, minlength=N).cpu().numpy()
        if counts.max() > per_call:
            raise ValueError(f"one image holds {counts.max()} meshes of {F} faces: more than {per_call} per image are not supported")
        groups, i0, n = [], 0, 0
        for i in range(N):
            if n + counts[i] > per_call:
                groups.append((i0, i, None))
                i0, n = i, 0
            n += counts[i]
        groups.append((i0, N, None))
        if len(groups) > 1:
            groups = [(a, b, torch.nonzero((img >= a) & (img < b)).flatten()) for a, b, _ in groups]
    l = _C.lib()
    for i0, i1, sel in groups:
        if img is None:
            gv, gT, gc, gimg, nb = v[i0:i1], T[i0:i1], col[i0:i1], None, i1 - i0
        elif sel is None:
            gv, gT, gc, gimg, nb = v, T, col, img.to(torch.int32).contiguous(), B
        else:
            gv, gT, gc = v[sel].contiguous(), T[sel].contiguous(), col[sel].contiguous()
            gimg, nb = (img[sel] - i0).to(torch.int32).contiguous(), int(sel.numel())
        ni = i1 - i0
        if nb == 0:                                                                 # images without meshes: background only
            gv, gT, gc, gimg, nb = v[:1], T[:1], col[:1], torch.zeros(1, dtype=torch.int32, device=dev), 1
            gv = torch.full_like(gv, float("nan"))                                   # (non-finite: every face dropped)
        scratch = torch.empty((int(l.dposer_render_scratch_bytes(nb, V, F, ni, H, W)),), dtype=torch.uint8, device=dev)
        ptr = lambda k: out[k][i0].data_ptr() if k in out else None
        a = _C.RenderArgs(vertices=gv.data_ptr(), num_meshes=nb, num_vertices=V, faces=f32.data_ptr(), num_faces=F, transforms=gT.data_ptr(),
                          image_of_mesh=None if gimg is None else gimg.data_ptr(), num_images=ni, height=H, width=W,
                          intrinsics=K[i0].data_ptr(), znear=float(znear), zfar=float(zfar), base_color=gc.data_ptr(),
                          lights=L.data_ptr() if L.shape[0] else None, num_lights=int(L.shape[0]), ambient=(C.c_float * 3)(*amb),
                          smooth=1 if smooth else 0, vf_ptr=None if vf_ptr is None else vf_ptr.data_ptr(),
                          vf_face=None if vf_face is None else vf_face.data_ptr(),
                          background=None if bg is None else (bg[i0] if bg.dim() == 4 else bg).data_ptr(), background_stride=bg_stride,
                          background_color=(C.c_uint8 * 4)(*bgc), rgb=ptr("rgb"), depth=ptr("depth"), face_id=ptr("face_id"),
                          mesh_id=ptr("mesh_id"), scratch=scratch.data_ptr())
        _C.check(l.dposer_render_meshes(C.byref(a), _C.stream_ptr()), "dposer_render_meshes")
        if sel is not None and sel.numel() and "mesh_id" in out:
            m = out["mesh_id"][i0:i1]
            m.copy_(torch.where(m >= 0, sel.to(torch.int32)[m.clamp_min(0).long()], m))
    return out


# ---- cameras of the reference's presets ----------------------------------------------------------------------------------------------
_GL_TO_CV = np.diag([1.0, -1.0, -1.0])


def rotation_x(deg):
    a = np.radians(deg)
    return np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])


def rotation_y(deg):
    a = np.radians(deg)
    return np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])


def parse_view(view):
    """(yaw, pitch) in degrees of render_mesh's view name (visual.py:144-176); 'random' draws the name with Python's ``random``."""
    if view == "random":
        chosen_side = random.choice(["half", ""])
        chosen_direction = random.choice(["left", "right", "front", "back"])
        chosen_height = random.choice(["above", "bottom", ""])
        view = "_".join([opt for opt in [chosen_side, chosen_direction, chosen_height] if opt])
    side_angle = 45 if "half" in view else 90
    if "left" in view:
        yaw = -side_angle
    elif "right" in view:
        yaw = side_angle
    elif "back" in view:
        yaw = 180
    else:
        yaw = 0
    pitch = 30 if "above" in view else (-30 if "bottom" in view else 0)
    return yaw, pitch


def render_mesh_transform(centroid, yaw, pitch):
    """[3, 4] model -> OpenCV camera of render_mesh: rotate about the centroid (yaw about y, then pitch about x), z -= 7, GL -> CV."""
    R = rotation_x(pitch) @ rotation_y(yaw)
    c = np.asarray(centroid, dtype=np.float64)
    t = c - R @ c + np.array([0.0, 0.0, -7.0])
    return np.concatenate([_GL_TO_CV @ R, (_GL_TO_CV @ t)[:, None]], 1)


def faster_camera():
    """(transform [3, 4], intrinsics [4]) of faster_render: pytorch3d's look_at_view_transform(2, 0, 0) with a 60-degree vertical field
    of view at 256 x 256 (camera at +2 on z looking at the origin, y up) in the OpenCV frame."""
    T = np.array([[1.0, 0, 0, 0], [0, -1.0, 0, 0], [0, 0, -1.0, 2.0]])
    f = (FASTER_SIZE / 2) / math.tan(math.radians(FASTER_FOV_DEG / 2))
    return T, np.array([f, f, FASTER_SIZE / 2, FASTER_SIZE / 2])


def renderer_lights():
    """Renderer's two directional lights (poses rotX(-45), rotY(45)): pyrender lights shine along the pose's -z, so the direction
    toward the light is the pose's +z axis, taken to the OpenCV frame."""
    dirs = [_GL_TO_CV @ rotation_x(-45)[:, 2], _GL_TO_CV @ rotation_y(45)[:, 2]]
    return [(0, *d, RENDERER_LIGHT, RENDERER_LIGHT, RENDERER_LIGHT) for d in dirs]


def _render_mesh_lights():
    # three lights whose poses only translate: all shine along the camera axis (pyrender: the pose's -z; toward the light = +z GL)
    return [(0, 0.0, 0.0, -1.0, RENDER_MESH_LIGHT, RENDER_MESH_LIGHT, RENDER_MESH_LIGHT)] * 3


def _to_gpu(x, dev):
    return x.detach().to(dev, torch.float32) if torch.is_tensor(x) else torch.as_tensor(np.asarray(x, dtype=np.float32), device=dev)


def _render_mesh_batch(meshes, faces, height, width, focal, princpt, views, dev):
    """render_mesh's scene for every mesh of ``meshes [B, V, 3]``, one image each: (rgb uint8 [B, H, W, 3], covered bool [B, H, W])."""
    v = _to_gpu(meshes, dev)
    B = v.shape[0]
    cent = v.double().mean(dim=1).cpu().numpy()
    T = np.stack([render_mesh_transform(cent[b], *parse_view(views[b])) for b in range(B)])
    K = [float(focal[0]), float(focal[1]), float(princpt[0]), float(princpt[1])]
    out = render_meshes(v, torch.as_tensor(np.asarray(faces) if not torch.is_tensor(faces) else faces, device=dev), K, (height, width),
                        transforms=torch.as_tensor(T, dtype=torch.float32, device=dev), base_color=RENDER_MESH_COLOR,
                        lights=_render_mesh_lights(), ambient=RENDER_MESH_AMBIENT, smooth=False, outputs=("rgb", "depth"))
    return out["rgb"], out["depth"] > 0


def render_mesh(img, mesh, face, cam_param, view="random"):
    """visual.py:132-214: ``mesh [V, 3]`` rendered over ``img [H, W, 3]``; float32 [H, W, 3], ``img`` wherever the mesh is absent."""
    img = np.asarray(img)
    rgb, mask = _render_mesh_batch(np.asarray(mesh)[None] if not torch.is_tensor(mesh) else mesh[None], face, img.shape[0], img.shape[1],
                                   cam_param["focal"], cam_param["princpt"], [view], _dev())
    rgb, mask = rgb[0].cpu().numpy().astype(np.float32), mask[0].cpu().numpy()
    return np.where(mask[:, :, None], rgb, img.astype(np.float32))


def _to_u8(a):
    return np.clip(np.rint(np.asarray(a, dtype=np.float64)), 0, 255).astype(np.uint8)


def multiple_render(samples, Normalizer, body_model, target_path, img_name, convert=True, idx_map=None, faster=True, device=None,
                    bg_img=None, focal=None, princpt=None, view="front"):
    """visual.py:231-250: every sample through one ``body_model`` forward and one render call; files ``img_name.format(idx + 1)``."""
    os.makedirs(target_path, exist_ok=True)
    assert len(samples.shape) == 2
    sample_num = samples.shape[0]
    if convert:
        samples = Normalizer.offline_denormalize(samples, to_axis=True)
    body_out = body_model(pose_body=samples)
    if faster:
        assert device is not None
        faster_render(body_out.v, body_out.f, target_path, img_name, device, idx_map)
        return
    bg = np.asarray(bg_img, dtype=np.float32)
    views = [view] * sample_num
    rgb, mask = _render_mesh_batch(body_out.v, body_out.f, bg.shape[0], bg.shape[1], focal, princpt, views, body_out.v.device)
    rgb, mask = rgb.cpu().numpy(), mask.cpu().numpy()
    for idx in range(sample_num):
        img = np.where(mask[idx][:, :, None], rgb[idx].astype(np.float32), bg)
        save_idx = idx if idx_map is None else idx_map[idx]
        write_image(os.path.join(target_path, img_name.format(save_idx + 1)), _to_u8(img))


def faster_render(vertices, faces, target_path, img_name, device, idx_map=None):
    """visual.py:253-287 (pytorch3d there): 256 x 256, 60-degree field of view, camera at distance 2 on +z, white smooth-shaded bodies
    lit by a point light at (0, 0, 3) over white."""
    os.makedirs(target_path, exist_ok=True)
    dev = torch.device(device) if device is not None else _dev()
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    v = _to_gpu(vertices, dev)
    T, K = faster_camera()
    light_cv = T[:, :3] @ np.array([0.0, 0.0, 3.0]) + T[:, 3]
    out = render_meshes(v, torch.as_tensor(faces, device=dev) if not torch.is_tensor(faces) else faces.to(dev), torch.as_tensor(K, dtype=torch.float32, device=dev),
                        (FASTER_SIZE, FASTER_SIZE), transforms=torch.as_tensor(T, dtype=torch.float32, device=dev), base_color=(1.0, 1.0, 1.0),
                        lights=[(1, *light_cv, FASTER_LIGHT, FASTER_LIGHT, FASTER_LIGHT)], ambient=FASTER_AMBIENT, smooth=True,
                        background_color=(255, 255, 255), znear=1.0, zfar=100.0, outputs=("rgb",))
    rgb = out["rgb"].cpu().numpy()
    for idx in range(len(v)):
        save_idx = idx if idx_map is None else idx_map[idx]
        write_image(os.path.join(target_path, img_name.format(save_idx + 1)), rgb[idx])


class Renderer(object):
    """visual.py:290-366 (CLIFF's renderer): every person of ``verts [n, V, 3]`` in one image at the origin camera.  The reference's
    180-degree flip about x and its GL camera compose to the identity in the OpenCV frame."""

    def __init__(self, focal_length=600, img_w=512, img_h=512, camera_center=None, faces=None, same_mesh_color=False):
        if camera_center is None:
            self.camera_center = [img_w // 2, img_h // 2]
        else:
            self.camera_center = camera_center
        self.focal_length = focal_length
        self.img_w, self.img_h = int(img_w), int(img_h)
        self.faces = faces
        self.same_mesh_color = same_mesh_color

    def render_front_view(self, verts, bg_img_rgb=None, bg_color=(0, 0, 0, 0)):
        dev = verts.device if torch.is_tensor(verts) and verts.is_cuda else _dev()
        v = _to_gpu(verts, dev)
        n = v.shape[0]
        if self.same_mesh_color:
            colors = [(0.4, 0.6, 0.93)] * n
        else:
            colors = [colorsys.hsv_to_rgb(float(k) / n, 0.5, 1.0) for k in range(n)]
        fl, cc = float(self.focal_length), [float(c) for c in self.camera_center]
        faces = self.faces if torch.is_tensor(self.faces) else torch.as_tensor(np.asarray(self.faces).astype(np.int64), device=dev)
        out = render_meshes(v, faces.to(dev), [fl, fl, cc[0], cc[1]], (self.img_h, self.img_w), image_of_mesh=torch.zeros(n, dtype=torch.int64, device=dev),
                            base_color=torch.as_tensor(colors, dtype=torch.float32, device=dev), lights=renderer_lights(), ambient=0.0, smooth=True,
                            background_color=_to_u8(np.asarray(bg_color[:3], dtype=np.float64) * 255), outputs=("rgb", "depth"))
        color_rgb = out["rgb"][0].cpu().numpy()
        if bg_img_rgb is None:
            return color_rgb
        mask = out["depth"][0].cpu().numpy() > 0
        bg_img_rgb[mask] = color_rgb[mask]
        return bg_img_rgb

    def render_side_view(self, verts):
        verts = verts.detach().cpu().numpy() if torch.is_tensor(verts) else np.asarray(verts)
        centroid = verts.mean(axis=(0, 1))
        centroid[:2] = 0
        aroundy = rotation_y(90.0)[np.newaxis, ...]                                # cv2.Rodrigues([0, pi/2, 0])
        pred_vert_arr_side = np.matmul((verts - centroid), aroundy) + centroid
        return self.render_front_view(pred_vert_arr_side)

    def delete(self):
        """No off-screen context to release (the reference's pyrender renderer needs this)."""


def save_obj(v, f, file_name="output.obj"):
    """visual.py:122-129, line for line."""
    with open(file_name, "w") as obj_file:
        for i in range(len(v)):
            obj_file.write("v " + str(v[i][0]) + " " + str(v[i][1]) + " " + str(v[i][2]) + "\n")
        for i in range(len(f)):
            obj_file.write("f " + str(f[i][0] + 1) + "/" + str(f[i][0] + 1) + " " + str(f[i][1] + 1) + "/" + str(f[i][1] + 1) + " " +
                           str(f[i][2] + 1) + "/" + str(f[i][2] + 1) + "\n")


def _png_chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def encode_png(rgb):
    """uint8 [H, W, 3] -> PNG bytes (8-bit RGB, filter 0 on every row), standard library only."""
    a = np.ascontiguousarray(rgb)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"encode_png takes uint8 [H, W, 3], got {a.dtype} {a.shape}")
    h, w = a.shape[:2]
    raw = np.concatenate([np.zeros((h, 1), np.uint8), a.reshape(h, w * 3)], 1).tobytes()
    return (b"\x89PNG\r\n\x1a\n" + _png_chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) +
            _png_chunk(b"IDAT", zlib.compress(raw, 6)) + _png_chunk(b"IEND", b""))


def write_image(path, rgb_uint8):
    """Write a uint8 [H, W, 3] RGB image: ``.png`` through the built-in writer, other extensions through PIL when it imports."""
    a = np.asarray(rgb_uint8)
    if os.path.splitext(path)[1].lower() == ".png":
        with open(path, "wb") as fh:
            fh.write(encode_png(a))
        return
    try:
        from PIL import Image
    except ImportError:
        raise RuntimeError(f"writing {path!r} needs PIL (only .png is written without it)") from None
    Image.fromarray(np.ascontiguousarray(a, dtype=np.uint8)).save(path)


# ---- skeleton plots (visual.py:18-119) -----------------------------------------------------------------------------------------------
SKELETON_SIZE = (480, 640)            # (H, W) of plt.savefig's default 6.4 x 4.8 in figure at 100 dpi
SKELETON_PADDING = 1.2                # visualize_skeleton_sequence's padding_ratio
LINE_WIDTH_PX = 2.0 * 100.0 / 72.0    # linewidth=2 (points) at 100 dpi
JOINT_RADIUS_PX = 3.0 * 100.0 / 72.0  # scatter's default marker: 6 pt across
SKELETON_FPS = 20.0

# matplotlib's 'rainbow' (256-entry table) at linspace(0, 1, 23)[:21], red and blue swapped as visual.py:35 swaps them; uint8 RGB
SKELETON_COLORS_21 = (
    (255, 0, 128), (254, 34, 106), (252, 71, 82), (249, 104, 60), (245, 137, 36), (239, 167, 12), (232, 192, 10), (224, 214, 34),
    (214, 232, 58), (204, 244, 80), (193, 252, 104), (180, 255, 128), (167, 252, 150), (152, 244, 174), (138, 232, 196),
    (122, 214, 220), (105, 192, 244), (89, 167, 255), (71, 137, 255), (53, 104, 255), (36, 71, 255))


def rainbow_swapped(n):
    """uint8 [n, 3]: matplotlib's ``rainbow`` colormap at ``linspace(0, 1, n + 2)[:n]`` with red and blue swapped -- the colours of
    visual.py:33-35 for n bones.  The colormap's three channel functions (|2x - 0.5|, sin(pi x), cos(pi x / 2), clipped to [0, 1]) sampled
    through its 256-entry table, as ``cmap(x)`` looks them up."""
    if n == len(SKELETON_COLORS_21):
        return np.asarray(SKELETON_COLORS_21, dtype=np.uint8)
    grid = np.linspace(0.0, 1.0, 256)
    lut = np.clip(np.stack([np.abs(2 * grid - 0.5), np.sin(np.pi * grid), np.cos(np.pi * grid / 2)], 1), 0.0, 1.0)
    x = np.linspace(0.0, 1.0, n + 2)[:n]
    idx = np.minimum((x * 256).astype(np.int64), 255)
    rgb = lut[idx]
    return np.rint(rgb[:, ::-1] * 255).astype(np.uint8)


def skeleton_joint_colors(bones, bone_color, num_joints):
    """uint8 [J, 3]: every joint in the colour of the last bone that touches it (the reference scatters both ends of bone l in colour l,
    later bones over earlier ones); joints no bone touches are black."""
    out = np.zeros((num_joints, 3), np.uint8)
    for (a, b), c in zip(np.asarray(bones).reshape(-1, 2), np.asarray(bone_color)):
        out[a] = c
        out[b] = c
    return out


def skeleton_view(lo, hi, image_size=SKELETON_SIZE, padding=SKELETON_PADDING, padded=False):
    """(s, X0, Y0, cx, cy) of the view that fits the bounds ``lo`` / ``hi`` [3]: the largest (padded) extent of the three axes spans
    min(H, W), the x / y centre of the bounds maps to the image centre.  ``padded``: the bounds already include the padding."""
    H, W = image_size
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    ext = float(np.max(hi - lo)) * (1.0 if padded else padding)
    s = min(H, W) / ext if ext > 0 and np.isfinite(ext) else 1.0
    return (s, float((lo[0] + hi[0]) / 2), float((lo[1] + hi[1]) / 2), W / 2.0, H / 2.0)


def draw_skeletons(joints, bones, image_size=SKELETON_SIZE, view=None, bone_color=None, joint_color=None, visible=None,
                   line_width=LINE_WIDTH_PX, joint_radius=JOINT_RADIUS_PX, background=None, background_color=(255, 255, 255), y_up=True,
                   z_toward_viewer=True):
    """Draw ``joints [B, J, 3]`` (device tensor) as ``bones [K, 2]`` and J discs: uint8 ``[B, H, W, 3]`` on the device, one
    ``dposer_draw_skeletons`` call (rules: the module docstring and include/dposer_hip.h).

    ``view`` = (s, X0, Y0, cx, cy): screen x = cx + s (X - X0), screen y = cy -/+ s (Y - Y0) (``y_up``); None fits the finite joints of
    the whole batch (``skeleton_view``).  ``bone_color`` uint8 [K, 3] (None: ``rainbow_swapped(K)``), ``joint_color`` uint8 [J, 3] (None:
    the last bone touching each joint), ``visible`` [J] (None: all).  ``background`` uint8 [H, W, 3] or [B, H, W, 3], else
    ``background_color``.  ROCm tensors only; no CPU fallback."""
    from .. import _C
    if not torch.is_tensor(joints):
        raise ValueError("joints must be a torch tensor on the GPU")
    _C.require_gpu(joints, "joints")
    dev = joints.device
    if joints.dim() != 3 or joints.shape[-1] != 3:
        raise ValueError(f"joints must be [B, J, 3], got {tuple(joints.shape)}")
    B, J = int(joints.shape[0]), int(joints.shape[1])
    H, W = (int(v) for v in image_size)
    if H < 1 or W < 1:
        raise ValueError(f"image_size must be >= 1 in both axes, got {(H, W)}")
    bones_np = np.asarray(bones.cpu() if torch.is_tensor(bones) else bones, dtype=np.int64).reshape(-1, 2)
    K = int(bones_np.shape[0])
    if K + J > _C.DRAW_MAX_PRIMITIVES:
        raise ValueError(f"{K} bones + {J} joints: more than {_C.DRAW_MAX_PRIMITIVES} primitives per frame are not supported")
    if K and (bones_np.min() < 0 or bones_np.max() >= J):
        raise ValueError(f"bone ends must lie in [0, {J})")
    bcol = rainbow_swapped(K) if bone_color is None else np.asarray(bone_color)
    if bcol.dtype != np.uint8 or bcol.shape != (K, 3):
        raise ValueError(f"bone_color must be uint8 [{K}, 3], got {bcol.dtype} {bcol.shape}")
    jcol = skeleton_joint_colors(bones_np, bcol, J) if joint_color is None else np.asarray(joint_color)
    if jcol.dtype != np.uint8 or jcol.shape != (J, 3):
        raise ValueError(f"joint_color must be uint8 [{J}, 3], got {jcol.dtype} {jcol.shape}")
    j = joints.detach().to(torch.float32).contiguous()
    out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev)
    if B == 0:
        return out
    if view is None:
        ok = torch.isfinite(j).all(dim=2)
        if visible is not None:
            ok = ok & torch.as_tensor(np.asarray(visible).reshape(-1) > 0, device=dev)[None, :]
        pts = j[ok]
        if pts.numel():
            view = skeleton_view(pts.min(dim=0).values.cpu().numpy(), pts.max(dim=0).values.cpu().numpy(), (H, W))
        else:
            view = (1.0, 0.0, 0.0, W / 2.0, H / 2.0)
    s, X0, Y0, cx, cy = (float(v) for v in view)
    vis_t = None if visible is None else torch.as_tensor((np.asarray(visible).reshape(-1) > 0).astype(np.uint8), device=dev)
    if vis_t is not None and vis_t.shape != (J,):
        raise ValueError(f"visible must be [{J}], got {tuple(vis_t.shape)}")
    bg, bg_stride = None, 0
    if background is not None:
        bg = torch.as_tensor(background, device=dev) if not torch.is_tensor(background) else background.to(dev)
        if bg.dtype != torch.uint8 or tuple(bg.shape[-3:]) != (H, W, 3) or bg.dim() not in (3, 4) or (bg.dim() == 4 and bg.shape[0] != B):
            raise ValueError(f"background must be uint8 [H, W, 3] or [B, H, W, 3], got {bg.dtype} {tuple(bg.shape)}")
        bg = bg.contiguous()
        bg_stride = H * W * 3 if bg.dim() == 4 else 0
    bgc = [int(c) for c in np.broadcast_to(np.asarray(background_color), (3,))] + [0]
    bones_t = torch.as_tensor(bones_np.astype(np.int32), device=dev).contiguous()
    bcol_t = torch.as_tensor(np.ascontiguousarray(bcol), device=dev)
    jcol_t = torch.as_tensor(np.ascontiguousarray(jcol), device=dev)
    l = _C.lib()
    tiles = -(-H // 16) * -(-W // 64)
    per_call = max(1, (2 ** 31 - 1) // tiles)
    for b0 in range(0, B, per_call):
        nb = min(B, b0 + per_call) - b0
        scratch = torch.empty((int(l.dposer_draw_skeletons_scratch_bytes(nb, J, K)),), dtype=torch.uint8, device=dev)
        a = _C.DrawSkeletonsArgs(joints=j[b0].data_ptr() if J else None, batch=nb, num_joints=J, num_bones=K,
                                 visible=None if vis_t is None else vis_t.data_ptr(), bones=bones_t.data_ptr() if K else None,
                                 bone_color=bcol_t.data_ptr() if K else None, joint_color=jcol_t.data_ptr() if J else None, s=s, X0=X0, Y0=Y0,
                                 cx=cx, cy=cy, y_up=1 if y_up else 0, z_toward_viewer=1 if z_toward_viewer else 0,
                                 line_width=float(line_width), joint_radius=float(joint_radius), height=H, width=W,
                                 background=None if bg is None else (bg[b0] if bg.dim() == 4 else bg).data_ptr(), background_stride=bg_stride,
                                 background_color=(C.c_uint8 * 4)(*bgc), rgb=out[b0].data_ptr(), scratch=scratch.data_ptr())
        _C.check(l.dposer_draw_skeletons(C.byref(a), _C.stream_ptr()), "dposer_draw_skeletons")
    return out


def _plot_frames(joints_np, kpt_3d_vis, kps_lines, ax_lims):
    """The frames of visualize_3d_skeleton for ``joints_np [B, J, 3]`` in its frame (the points vis_skeletons has flipped about x: the
    figure shows x to the right, -y up, and a larger z farther): uint8 [B, 480, 640, 3] on the device."""
    dev = _dev()
    j = torch.as_tensor(np.asarray(joints_np, dtype=np.float32), device=dev)
    vis = None if kpt_3d_vis is None else np.asarray(kpt_3d_vis).reshape(len(kpt_3d_vis), -1)[:, 0] > 0
    view = None if ax_lims is None else skeleton_view([ax_lims[0], ax_lims[2], ax_lims[4]], [ax_lims[1], ax_lims[3], ax_lims[5]], padded=True)
    return draw_skeletons(j, np.asarray(kps_lines), view=view, visible=vis, y_up=False, z_toward_viewer=False)


def visualize_3d_skeleton(kpt_3d, kpt_3d_vis, kps_lines, title=None, output_path=None, ax_lims=None):
    """visual.py:18-64: one skeleton frame ``kpt_3d [J, 3]``; written to ``output_path`` when given (the reference opens a window
    otherwise) and returned as uint8 [480, 640, 3].  ``title`` is accepted and ignored."""
    img = _plot_frames(np.asarray(kpt_3d)[None], kpt_3d_vis, kps_lines, ax_lims)[0].cpu().numpy()
    if output_path:
        write_image(output_path, img)
    return img


def visualize_skeleton_sequence(joints_seq, kpt_3d_vis, kps_lines, output_path):
    """visual.py:67-104: every frame of ``joints_seq [T, J, 3]`` under one view, drawn in one call.  A path ending in ``.mp4`` gets a
    20 fps video (written as ``.avi``, see ``utils.motion_video.write_video``; the real path is returned), a path without extension is
    a directory of ``frame_%04d.png``; anything else raises the reference's ValueError."""
    joints_seq = np.asarray(joints_seq)
    is_video = output_path.endswith(".mp4")
    if not is_video and os.path.splitext(output_path)[1]:
        raise ValueError("The output_path must end with .mp4 or no extension!")
    pts = joints_seq.reshape(-1, 3)
    joint_min, joint_max = np.min(pts, axis=0), np.max(pts, axis=0)
    center, half = (joint_max + joint_min) / 2, SKELETON_PADDING * (joint_max - joint_min) / 2
    ax_lims = [center[0] - half[0], center[0] + half[0], center[1] - half[1], center[1] + half[1], center[2] - half[2], center[2] + half[2]]
    frames = _plot_frames(joints_seq, kpt_3d_vis, kps_lines, ax_lims)
    if is_video:
        from ..utils.motion_video import write_video
        return write_video(output_path, frames, SKELETON_FPS)
    os.makedirs(output_path, exist_ok=True)
    rgb = frames.cpu().numpy()
    for i in range(len(rgb)):
        write_image(os.path.join(output_path, f"frame_{i:04d}.png"), rgb[i])
    return output_path


def vis_skeletons(joints_3d, output_path):
    """visual.py:107-119: 22 SMPL joints, one frame ``[22, 3]`` or a sequence ``[T, 22, 3]``, as an upright front view."""
    from ..utils.transforms import get_rotation_matrix_x, rotate_points
    from .utils import get_smpl_skeleton
    joints_3d = rotate_points(np.asarray(joints_3d), get_rotation_matrix_x(np.pi))
    kpt_3d_vis = np.ones((22, 1))
    kps_lines = get_smpl_skeleton()
    if len(joints_3d.shape) == 2:
        visualize_3d_skeleton(joints_3d, kpt_3d_vis, kps_lines, output_path=output_path)
    elif len(joints_3d.shape) == 3:
        visualize_skeleton_sequence(joints_3d, kpt_3d_vis, kps_lines, output_path)
