"""lib/utils/motion_video.py: the three-panel motion-denoising video (noisy joints, result, ground truth) and the video writer behind every
``.mp4`` the reference's scripts produce.

The reference composites one frame at a time with numpy / cv2 and encodes with ``cv2.VideoWriter``; here all N frames of a sequence are
composed in one ``dposer_compose_panels`` call (csrc/draw.hip; rules in include/dposer_hip.h) and written as an uncompressed AVI by
``write_video`` (standard library + numpy: this package carries no codec).  A requested path that does not end in ``.avi`` has its
suffix replaced; the real path is returned and printed.  Images are RGB throughout (the reference handles BGR arrays from ``cv2.imread``;
the files look the same).  Title strips are drawn once on the host with PIL's built-in font (cv2's Hershey text is not reproduced;
without PIL the strips are blank).  ``process_image`` / ``crop`` of the reference's preprocess module are not part of this file.
"""
import ctypes as C
import math
import os
import struct

import numpy as np
import torch

PANEL_W, PANEL_H = 256, 400           # resize_or_crop's target in process_body / process_joint
TITLE_H = 30                          # add_title's blank_height
BODY_CROP_BOTTOM = 20                 # process_body's default
JOINT_SCALE = 0.9                     # process_joint's resize factor
WHITE = (255, 255, 255)


def _dev():
    return torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")


def _frames_on_device(x, name):
    """uint8 [N, H, W, 3] contiguous on the GPU from a device tensor or an array ([H, W, 3] becomes one frame)."""
    from .. import _C
    t = x if torch.is_tensor(x) else torch.as_tensor(np.ascontiguousarray(x), device=_dev())
    _C.require_gpu(t, name)
    if t.dim() == 3:
        t = t[None]
    if t.dtype != torch.uint8 or t.dim() != 4 or t.shape[-1] != 3 or t.shape[1] < 1 or t.shape[2] < 1:
        raise ValueError(f"{name} must be uint8 [N, H, W, 3], got {t.dtype} {tuple(t.shape)}")
    return t.contiguous()


def compose_panels(panels, num_frames, out_size, out_fill=WHITE):
    """``num_frames`` frames uint8 ``[N, out_h, out_w, 3]`` (device) from ``panels`` in one ``dposer_compose_panels`` call.  A panel is a
    dict: ``src`` uint8 [N or 1, Hs, Ws, 3] device tensor; ``crop`` (x, y, w, h) (default: all); ``resize`` (Hr, Wr) (default: the crop:
    no resampling); ``cell`` (Hp, Wp); ``fill`` RGB (default white); ``strip`` uint8 [Ht, Wp, 3] or None; ``x`` the cell's x offset."""
    from .. import _C
    out_h, out_w = (int(v) for v in out_size)
    N = int(num_frames)
    if len(panels) > _C.MAX_PANELS:
        raise ValueError(f"at most {_C.MAX_PANELS} panels per call, got {len(panels)}")
    arr = (_C.Panel * max(1, len(panels)))()
    keep, dev = [], None
    for k, p in enumerate(panels):
        src = _frames_on_device(p["src"], "a panel's src")
        dev = dev or src.device
        if src.device != dev:
            raise ValueError("every panel must live on the same device")
        if src.shape[0] not in (1, N):
            raise ValueError(f"a panel's src must hold 1 or {N} frames, got {src.shape[0]}")
        Hs, Ws = int(src.shape[1]), int(src.shape[2])
        x, y, w, h = (int(v) for v in p.get("crop", (0, 0, Ws, Hs)))
        Hr, Wr = (int(v) for v in p.get("resize", (h, w)))
        Hp, Wp = (int(v) for v in p["cell"])
        strip = p.get("strip")
        if strip is not None:
            strip = torch.as_tensor(np.ascontiguousarray(strip), device=dev) if not torch.is_tensor(strip) else strip.to(dev).contiguous()
            if strip.dtype != torch.uint8 or strip.dim() != 3 or strip.shape[1] != Wp or strip.shape[2] != 3:
                raise ValueError(f"a strip must be uint8 [Ht, {Wp}, 3], got {strip.dtype} {tuple(strip.shape)}")
        keep += [src, strip]
        fill = [int(c) for c in np.broadcast_to(np.asarray(p.get("fill", WHITE)), (3,))] + [0]
        arr[k] = _C.Panel(src=src.data_ptr(), src_stride=Hs * Ws * 3 if src.shape[0] > 1 else 0, src_h=Hs, src_w=Ws, crop_x=x, crop_y=y,
                          crop_w=w, crop_h=h, resize_h=Hr, resize_w=Wr, cell_h=Hp, cell_w=Wp, fill=(C.c_uint8 * 4)(*fill),
                          strip=None if strip is None or strip.shape[0] == 0 else strip.data_ptr(),
                          strip_h=0 if strip is None else int(strip.shape[0]), x_offset=int(p.get("x", 0)))
    dev = dev or _dev()
    out = torch.empty((N, out_h, out_w, 3), dtype=torch.uint8, device=dev)
    _C.require_gpu(out, "the output")
    fill = [int(c) for c in np.broadcast_to(np.asarray(out_fill), (3,))] + [0]
    a = _C.ComposeArgs(panels=arr, num_panels=len(panels), num_frames=N, out_h=out_h, out_w=out_w, out_fill=(C.c_uint8 * 4)(*fill),
                       out=out.data_ptr())
    _C.check(_C.lib().dposer_compose_panels(C.byref(a), _C.stream_ptr()), "dposer_compose_panels")
    return out


def _as_array(img, out):
    """numpy in -> numpy out (the reference's functions take and return arrays); a device tensor stays on the device."""
    return out if torch.is_tensor(img) else out.cpu().numpy()


def resize_or_crop(input_img, width, height):
    """motion_video.py:6-29: ``input_img [h, w, 3]`` placed into ``height x width``: a wider image keeps its centre columns, a narrower
    one is centred over white; a taller image keeps its bottom rows, a shorter one is bottom-aligned over white.  The two axes are
    handled independently (the reference raises a numpy shape error for a narrow image of another height).  An exact byte move."""
    src = _frames_on_device(input_img, "input_img")
    out = compose_panels([dict(src=src, cell=(height, width))], src.shape[0], (height, width))
    return _as_array(input_img, out[0] if input_img.ndim == 3 else out)


def crop_bottom(input_img, crop_length):
    """motion_video.py:32-38: ``input_img`` without its last ``crop_length`` rows."""
    src = _frames_on_device(input_img, "input_img")
    h, w = int(src.shape[1]), int(src.shape[2])
    keep = len(range(h)[0:h - int(crop_length)])                                # (numpy's img[0:h - crop_length])
    if keep == 0:
        out = torch.empty((src.shape[0], 0, w, 3), dtype=torch.uint8, device=src.device)
    else:
        out = compose_panels([dict(src=src, crop=(0, 0, w, keep), cell=(keep, w))], src.shape[0], (keep, w))
    return _as_array(input_img, out[0] if input_img.ndim == 3 else out)


def _read_rgb(path):
    try:
        from PIL import Image
    except ImportError:
        raise RuntimeError(f"reading {path!r} needs PIL") from None
    return np.asarray(Image.open(path).convert("RGB"))


def _body_panel(src, x, strip=None, bottom=BODY_CROP_BOTTOM):
    h, w = int(src.shape[1]), int(src.shape[2])
    return dict(src=src, crop=(0, 0, w, h - bottom), cell=(PANEL_H, PANEL_W), strip=strip, x=x)


def _joint_panel(src, x, strip=None):
    h, w = int(src.shape[1]), int(src.shape[2])
    return dict(src=src, resize=(int(h * JOINT_SCALE), int(w * JOINT_SCALE)), cell=(PANEL_H, PANEL_W), strip=strip, x=x)


def process_body(body_img_path, bottom=20):
    """motion_video.py:41-45: a rendered body without its ``bottom`` rows, placed into 256 x 400; uint8 [400, 256, 3] RGB."""
    src = _frames_on_device(_read_rgb(body_img_path), body_img_path)
    return compose_panels([_body_panel(src, 0, bottom=bottom)], 1, (PANEL_H, PANEL_W))[0].cpu().numpy()


def process_joint(joint_img_path):
    """motion_video.py:48-55: a skeleton frame resized to 0.9 (bilinear, cv2.INTER_LINEAR's geometry), placed into 256 x 400."""
    src = _frames_on_device(_read_rgb(joint_img_path), joint_img_path)
    return compose_panels([_joint_panel(src, 0)], 1, (PANEL_H, PANEL_W))[0].cpu().numpy()


def title_strip(text, width=PANEL_W, height=TITLE_H):
    """uint8 [height, width, 3]: ``text`` in black, centred on white, PIL's built-in font; blank without PIL."""
    blank = np.full((height, width, 3), 255, np.uint8)
    if not text:
        return blank
    try:
        from PIL import Image, ImageDraw, ImageFont
    except ImportError:
        return blank
    img = Image.fromarray(blank)
    draw = ImageDraw.Draw(img)
    font = ImageFont.load_default()
    l, t, r, b = draw.textbbox((0, 0), text, font=font)
    draw.text(((width - (r - l)) // 2 - l, (height - (b - t)) // 2 - t), text, fill=(0, 0, 0), font=font)
    return np.asarray(img).copy()


_TITLES = {}


def _title_on_device(text, dev):
    """``title_strip(text)`` on ``dev``, made and uploaded once per (text, device)."""
    key = (text, str(dev))
    if key not in _TITLES:
        _TITLES[key] = torch.as_tensor(title_strip(text), device=dev)
    return _TITLES[key]


def compose_motion_frames(skeleton_frames, out_frames, gt_frames, titles=("Noisy Joints", "DPoser(Ours)", "GT")):
    """The merged frames of ``seq_to_video`` (motion_video.py:111-126) for a whole sequence in one call: uint8 device tensors
    ``skeleton_frames [N, Hj, Wj, 3]`` (``process_joint``), ``out_frames`` and ``gt_frames [N, Hb, Wb, 3]`` (``process_body``) ->
    ``[N, 430, 768, 3]``: three 256 x 400 cells side by side, a 30-row title strip under each."""
    sk = _frames_on_device(skeleton_frames, "skeleton_frames")
    ou = _frames_on_device(out_frames, "out_frames")
    gt = _frames_on_device(gt_frames, "gt_frames")
    N = int(sk.shape[0])
    if ou.shape[0] != N or gt.shape[0] != N:
        raise ValueError(f"the three panels must hold the same number of frames, got {N}, {ou.shape[0]}, {gt.shape[0]}")
    strips = [_title_on_device(str(t), sk.device) for t in titles]
    panels = [_joint_panel(sk, 0, strips[0]), _body_panel(ou, PANEL_W, strips[1]), _body_panel(gt, 2 * PANEL_W, strips[2])]
    return compose_panels(panels, N, (PANEL_H + TITLE_H, 3 * PANEL_W))


# ---- uncompressed AVI -----------------------------------------------------------------------------------------------------------------
# RIFF 'AVI ' { LIST 'hdrl' { 'avih', LIST 'strl' { 'strh' ('vids' / 'DIB '), 'strf' (BITMAPINFOHEADER, 24-bit BI_RGB) } },
#               LIST 'movi' { one '00db' chunk per frame: bottom-up BGR rows padded to 4 bytes }, 'idx1' }
# idx1 offsets count from the 'movi' fourcc (the first chunk sits at 4), as the AVI 1.0 index does.
_AVIF_HASINDEX, _AVIIF_KEYFRAME = 0x10, 0x10
_RIFF_MAX = (1 << 32) - 1


def _chunk(fourcc, data):
    return fourcc + struct.pack("<I", len(data)) + data + (b"\x00" if len(data) & 1 else b"")


def _rate_scale(fps):
    scale = 1000
    rate = int(round(float(fps) * scale))
    g = math.gcd(rate, scale)
    return rate // g, scale // g


def avi_path(path):
    """The path ``write_video`` writes for a requested ``path``: its suffix replaced by ``.avi``."""
    root, ext = os.path.splitext(path)
    return path if ext.lower() == ".avi" else root + ".avi"


def write_video(path, frames, fps):
    """Write ``frames`` uint8 ``[N, H, W, 3]`` RGB (array or tensor, any device) as an uncompressed AVI at ``fps``.  A path that does not end
    in ``.avi`` has its suffix replaced (no MPEG-4 codec here); the path written is printed and returned."""
    a = frames.detach().cpu().numpy() if torch.is_tensor(frames) else np.asarray(frames)
    if a.dtype != np.uint8 or a.ndim != 4 or a.shape[3] != 3 or a.shape[1] < 1 or a.shape[2] < 1:
        raise ValueError(f"write_video takes uint8 [N, H, W, 3], got {a.dtype} {a.shape}")
    if not (float(fps) > 0 and math.isfinite(float(fps))):
        raise ValueError(f"fps must be positive, got {fps}")
    N, H, W = a.shape[:3]
    stride = (W * 3 + 3) & ~3
    frame_bytes = stride * H
    rate, scale = _rate_scale(fps)
    if rate < 1:
        raise ValueError(f"fps {fps} is too small")
    avih = struct.pack("<14I", int(round(1e6 * scale / rate)), min(_RIFF_MAX, int(math.ceil(frame_bytes * rate / scale))), 0, _AVIF_HASINDEX,
                       N, 0, 1, frame_bytes, W, H, 0, 0, 0, 0)
    strh = b"vids" + b"DIB " + struct.pack("<IHHIIIIIIII4h", 0, 0, 0, 0, scale, rate, 0, N, frame_bytes, 0xFFFFFFFF, 0, 0, 0, W, H)
    strf = struct.pack("<IiiHHIIiiII", 40, W, H, 1, 24, 0, frame_bytes, 0, 0, 0, 0)
    strl = b"LIST" + struct.pack("<I", 4 + len(_chunk(b"strh", strh)) + len(_chunk(b"strf", strf))) + b"strl" + _chunk(b"strh", strh) + _chunk(b"strf", strf)
    hdrl = b"LIST" + struct.pack("<I", 4 + len(_chunk(b"avih", avih)) + len(strl)) + b"hdrl" + _chunk(b"avih", avih) + strl
    movi_size = 4 + N * (8 + frame_bytes)
    idx1 = b"".join(struct.pack("<4sIII", b"00db", _AVIIF_KEYFRAME, 4 + i * (8 + frame_bytes), frame_bytes) for i in range(N))
    riff_size = 4 + len(hdrl) + 8 + movi_size + 8 + len(idx1)
    if riff_size > _RIFF_MAX:
        raise ValueError(f"{N} frames of {W} x {H} need {riff_size} bytes: more than one RIFF file holds (write fewer frames per file)")
    path = avi_path(path)
    row = np.zeros((H, stride), np.uint8)
    with open(path, "wb") as fh:
        fh.write(b"RIFF" + struct.pack("<I", riff_size) + b"AVI " + hdrl + b"LIST" + struct.pack("<I", movi_size) + b"movi")
        head = b"00db" + struct.pack("<I", frame_bytes)
        for i in range(N):
            row[:, :W * 3] = a[i, ::-1, :, ::-1].reshape(H, W * 3)
            fh.write(head)
            fh.write(row.tobytes())
        fh.write(b"idx1" + struct.pack("<I", len(idx1)) + idx1)
    print(f"Video {path} created successfully!")
    return path


def read_video(path):
    """The inverse of ``write_video``: (frames uint8 [N, H, W, 3] RGB, fps) of an uncompressed 24-bit AVI."""
    with open(path, "rb") as fh:
        data = fh.read()
    if data[:4] != b"RIFF" or data[8:12] != b"AVI ":
        raise ValueError(f"{path!r} is not a RIFF AVI file")
    info, frames = {}, []

    def walk(lo, hi):
        while lo + 8 <= hi:
            cc, size = data[lo:lo + 4], struct.unpack_from("<I", data, lo + 4)[0]
            body = lo + 8
            if cc == b"LIST":
                walk(body + 4, body + size)
            elif cc == b"strh":
                info["scale"], info["rate"] = struct.unpack_from("<II", data, body + 20)
            elif cc == b"strf":
                _, w, h, _, bits, comp = struct.unpack_from("<IiiHHI", data, body)
                info.update(w=w, h=h, bits=bits, comp=comp)
            elif cc in (b"00db", b"00dc"):
                frames.append((body, size))
            lo = body + size + (size & 1)

    walk(12, min(len(data), 8 + struct.unpack_from("<I", data, 4)[0]))
    if info.get("bits") != 24 or info.get("comp") != 0 or "rate" not in info:
        raise ValueError(f"{path!r}: only uncompressed 24-bit AVI files are read")
    W, H = info["w"], abs(info["h"])
    stride = (W * 3 + 3) & ~3
    out = np.empty((len(frames), H, W, 3), np.uint8)
    for i, (at, size) in enumerate(frames):
        if size != stride * H:
            raise ValueError(f"{path!r}: frame {i} holds {size} bytes, expected {stride * H}")
        rows = np.frombuffer(data, np.uint8, size, at).reshape(H, stride)[:, :W * 3].reshape(H, W, 3)
        out[i] = (rows[::-1] if info["h"] > 0 else rows)[:, :, ::-1]
    return out, info["rate"] / info["scale"]


def images_to_video(input_folder, output_file, fps=20):
    """motion_video.py:58-86: the ``merge_*.png`` files of ``input_folder``, sorted, as one video (``write_video``'s path is returned)."""
    images = sorted([os.path.join(input_folder, f) for f in os.listdir(input_folder) if f.startswith("merge_") and f.endswith(".png")])
    if not images:
        print("No images found in the specified directory!")
        return None
    return write_video(output_file, np.stack([_read_rgb(p) for p in images]), fps)


def seq_to_video(img_folder_path, output_merge_folder, video_path):
    """motion_video.py:89-130: ``frame_/out_/gt_%04d.png`` of ``img_folder_path`` -> ``merge_%04d.png`` in ``output_merge_folder`` and
    the video; every frame is composed in one call (``compose_motion_frames``)."""
    from ..body_model.visual import write_image
    img_number = len(os.listdir(img_folder_path))
    os.makedirs(output_merge_folder, exist_ok=True)
    n = img_number // 3
    if n:
        read = lambda stem: np.stack([_read_rgb(os.path.join(img_folder_path, "{}_{:04d}.png".format(stem, i))) for i in range(n)])
        merged = compose_motion_frames(read("frame"), read("out"), read("gt")).cpu().numpy()
        for i in range(n):
            write_image(os.path.join(output_merge_folder, "merge_{:04d}.png".format(i)), merged[i])
    return images_to_video(output_merge_folder, video_path)
