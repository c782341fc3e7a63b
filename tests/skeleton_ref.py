"""fp64 restatement of the drawing rules of include/dposer_hip.h (dposer_draw_skeletons, dposer_compose_panels) from fp32 inputs:
the oracle of tests/test_gpu_draw.py.  numpy only; nothing here imports the package."""
import numpy as np


def project(joints, view, y_up=True, z_toward_viewer=True):
    """joints fp32 [B, J, 3] -> (screen x, screen y, depth) in fp64; a larger depth is farther."""
    s, X0, Y0, cx, cy = (float(np.float32(v)) for v in view)
    j = np.asarray(joints, np.float32).astype(np.float64)
    sx = cx + s * (j[..., 0] - X0)
    sy = cy - s * (j[..., 1] - Y0) if y_up else cy + s * (j[..., 1] - Y0)
    depth = -j[..., 2] if z_toward_viewer else j[..., 2]
    return sx, sy, depth


def frame_keys(joints_frame, bones, z_toward_viewer=True):
    """(keys [K + J], valid [K + J]) of one frame; validity here covers finiteness only (visibility does not change a key)."""
    j = np.asarray(joints_frame, np.float32).astype(np.float64)
    fin = np.isfinite(j).all(axis=1)
    depth = -j[:, 2] if z_toward_viewer else j[:, 2]
    bones = np.asarray(bones).reshape(-1, 2)
    with np.errstate(invalid="ignore"):
        bk = 0.5 * (depth[bones[:, 0]] + depth[bones[:, 1]])
    bv = fin[bones[:, 0]] & fin[bones[:, 1]]
    return np.concatenate([np.where(bv, bk, 0.0), np.where(fin, depth - 1e-3, 0.0)]), np.concatenate([bv, fin])


def min_key_gap(joints, bones, visible=None, z_toward_viewer=True):
    """The smallest gap between the depth keys of two drawn primitives of one frame, over the batch (the one discrete decision)."""
    joints = np.asarray(joints, np.float32)
    bones = np.asarray(bones).reshape(-1, 2)
    J = joints.shape[1]
    vis = np.ones(J, bool) if visible is None else np.asarray(visible).reshape(-1) > 0
    drawn = np.concatenate([vis[bones[:, 0]] & vis[bones[:, 1]], vis])
    gap = np.inf
    for b in range(joints.shape[0]):
        k, v = frame_keys(joints[b], bones, z_toward_viewer)
        k = np.sort(k[v & drawn])
        if len(k) > 1:
            gap = min(gap, float(np.min(np.diff(k))))
    return gap


def draw_skeletons(joints, bones, bone_color, joint_color, view, hw, visible=None, line_width=2.0, joint_radius=3.0, background=None,
                   background_color=(255, 255, 255), y_up=True, z_toward_viewer=True):
    """uint8 [B, H, W, 3] and the unrounded fp64 image (for 'how close to a rounding boundary')."""
    joints = np.asarray(joints, np.float32)
    bones = np.asarray(bones).reshape(-1, 2)
    B, J = joints.shape[:2]
    K = len(bones)
    H, W = hw
    vis = np.ones(J, bool) if visible is None else np.asarray(visible).reshape(-1) > 0
    sx, sy, _ = project(joints, view, y_up, z_toward_viewer)
    lw, jr = float(np.float32(line_width)), float(np.float32(joint_radius))
    px, py = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    out = np.empty((B, H, W, 3), np.float64)
    for b in range(B):
        if background is None:
            c = np.broadcast_to(np.asarray(background_color, np.float64), (H, W, 3)).copy()
        else:
            bg = np.asarray(background)
            c = (bg[b] if bg.ndim == 4 else bg).astype(np.float64)
        keys, fin = frame_keys(joints[b], bones, z_toward_viewer)
        order = sorted(range(K + J), key=lambda p: (-keys[p], p))             # far to near, ties in primitive index order
        for p in order:
            if not fin[p]:
                continue
            if p < K:
                j0, j1 = bones[p]
                r, col = lw / 2, np.asarray(bone_color[p], np.float64)
            else:
                j0 = j1 = p - K
                r, col = jr, np.asarray(joint_color[p - K], np.float64)
            if not (vis[j0] and vis[j1]):
                continue
            ax, ay, bx, by = sx[b, j0], sy[b, j0], sx[b, j1], sy[b, j1]
            if not all(np.isfinite(v) for v in (ax, ay, bx, by)):
                continue
            # only the pixels whose centres lie within r + 0.5 of the primitive's box can be covered: the rest keep a = 0
            pad = r + 1.5
            x0, x1 = int(np.clip(np.floor(min(ax, bx) - pad), 0, W)), int(np.clip(np.ceil(max(ax, bx) + pad), 0, W))
            y0, y1 = int(np.clip(np.floor(min(ay, by) - pad), 0, H)), int(np.clip(np.ceil(max(ay, by) + pad), 0, H))
            if x0 >= x1 or y0 >= y1:
                continue
            qx, qy = px[y0:y1, x0:x1], py[y0:y1, x0:x1]
            ex, ey = bx - ax, by - ay
            l2 = ex * ex + ey * ey
            t = np.clip(((qx - ax) * ex + (qy - ay) * ey) / l2, 0.0, 1.0) if l2 > 0 else np.zeros_like(qx)
            d = np.hypot(qx - ax - t * ex, qy - ay - t * ey)
            a = np.clip(r + 0.5 - d, 0.0, 1.0)[..., None]
            c[y0:y1, x0:x1] = c[y0:y1, x0:x1] * (1 - a) + col * a
        out[b] = c
    return np.rint(out).astype(np.uint8), out


def place(img, width, height, fill=(255, 255, 255)):
    """resize_or_crop with the two axes handled independently (the header's placement rule), numpy, exact."""
    h, w = img.shape[:2]
    out = np.empty((height, width, 3), np.uint8)
    out[:] = np.asarray(fill, np.uint8)
    if w > width:
        left = (w - width) // 2
        img = img[:, left:left + width]
        x0 = 0
    else:
        x0 = (width - w) // 2
    if h > height:
        img = img[h - height:]
        y0 = 0
    else:
        y0 = height - h
    out[y0:y0 + img.shape[0], x0:x0 + img.shape[1]] = img
    return out


def resize_bilinear(img, hr, wr):
    """The documented cv2.INTER_LINEAR geometry in fp64: (rounded uint8, unrounded fp64)."""
    h, w = img.shape[:2]
    a = img.astype(np.float64)

    def taps(n_dst, n_src):
        scale = float(np.float32(n_src) / np.float32(n_dst))
        u = (np.arange(n_dst) + 0.5) * scale - 0.5
        i0 = np.floor(u)
        f = u - i0
        lo = np.clip(i0, 0, n_src - 1).astype(int)
        hi = np.clip(i0 + 1, 0, n_src - 1).astype(int)
        return lo, hi, f

    ya, yb, fy = taps(hr, h)
    xa, xb, fx = taps(wr, w)
    fx = fx[None, :, None]
    fy = fy[:, None, None]
    top = (1 - fx) * a[ya][:, xa] + fx * a[ya][:, xb]
    bot = (1 - fx) * a[yb][:, xa] + fx * a[yb][:, xb]
    v = (1 - fy) * top + fy * bot
    return np.rint(v).astype(np.uint8), v


def compose(panels, n_frames, out_hw, out_fill=(255, 255, 255)):
    """Exact-path compositor (no resampling): panels are dicts as utils.motion_video.compose_panels takes them, with numpy sources."""
    H, W = out_hw
    out = np.empty((n_frames, H, W, 3), np.uint8)
    out[:] = np.asarray(out_fill, np.uint8)
    for p in panels:
        src = np.asarray(p["src"])
        hs, ws = src.shape[1:3]
        x, y, w, h = p.get("crop", (0, 0, ws, hs))
        hp, wp = p["cell"]
        x0 = p.get("x", 0)
        for n in range(n_frames):
            img = src[n if src.shape[0] > 1 else 0][y:y + h, x:x + w]
            if "resize" in p and tuple(p["resize"]) != (h, w):
                img = resize_bilinear(img, *p["resize"])[0]
            out[n, :hp, x0:x0 + wp] = place(img, wp, hp, p.get("fill", (255, 255, 255)))
            if p.get("strip") is not None:
                st = np.asarray(p["strip"])
                out[n, hp:hp + st.shape[0], x0:x0 + wp] = st
    return out


def random_sequence(seed, frames, spread=(0.35, 0.5, 4.0)):
    """fp32 [frames, 22, 3]: a random 22-joint skeleton drifting over the sequence with per-frame jitter.  The depth axis is spread wider
    than the other two (the view is orthographic: depth only orders the primitives), which keeps the 43 depth keys of a frame apart."""
    rs = np.random.RandomState(seed)
    base = rs.standard_normal((22, 3)) * np.asarray(spread)
    drift = rs.standard_normal((22, 3)) * 0.15
    t = np.linspace(0.0, 1.0, frames)[:, None, None]
    return (base + drift * t + rs.standard_normal((frames, 22, 3)) * 0.02).astype(np.float32)
