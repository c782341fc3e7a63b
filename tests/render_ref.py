"""Test infrastructure: the rasterisation and shading rules of dposer_render_meshes (include/dposer_hip.h) restated in numpy fp64,
vectorised per triangle over its pixel box (triangles many at a time on square stencils of 8, 16, 32 ... pixels).

Besides the result it marks a pixel ambiguous when the fp32 kernel may legitimately decide it otherwise:
    - the centre lies within MARGIN_REL * max(H, W) pixels of an edge of a triangle (inside or out) whose depth there is not behind
      the winner's (the winner itself, the runner-up, or a triangle that may cover it in fp32);
    - the two nearest depths there agree to DEPTH_REL relative.
The GPU's face_id / mesh_id must equal the oracle on every pixel that is not ambiguous."""
import struct
import zlib

import numpy as np

MARGIN_REL = 4e-6
DEPTH_REL = 2e-6
SMALL = 8                   # smallest stencil edge


def project(vertices, transforms, intrinsics_of_mesh):
    """fp64 camera-frame positions and (u, v, z) of float32 inputs: [B, V, 3] each."""
    v = np.asarray(vertices, np.float32).astype(np.float64)
    T = np.asarray(transforms, np.float32).astype(np.float64)
    cam = np.einsum("bij,bvj->bvi", T[:, :, :3], v) + T[:, None, :, 3]
    K = np.asarray(intrinsics_of_mesh, np.float32).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        u = K[:, None, 0] * cam[..., 0] / cam[..., 2] + K[:, None, 2]
        w = K[:, None, 1] * cam[..., 1] / cam[..., 2] + K[:, None, 3]
    return cam, np.stack([u, w, cam[..., 2]], -1)


def _edges(P):
    """oriented edge data of triangles P [n, 3, 3] (screen u, v, z): start points A [n, 3, 2], directions D [n, 3, 2] with the interior
    positive, top-left ownership own [n, 3]."""
    A = P[:, :, :2]
    Bp = np.roll(A, -1, axis=1)
    area = (P[:, 1, 0] - P[:, 0, 0]) * (P[:, 2, 1] - P[:, 0, 1]) - (P[:, 1, 1] - P[:, 0, 1]) * (P[:, 2, 0] - P[:, 0, 0])
    D = (Bp - A) * np.sign(area)[:, None, None]
    own = (D[..., 1] < 0) | ((D[..., 1] == 0) & (D[..., 0] > 0))
    return A, D, own, area


def _eval(P, A, D, own, px, py, margin):
    """fragments of triangles on pixel centres px, py [n, k]: (strict cover, near-edge, z) [n, k], and the edge values [n, k, 3]."""
    w = D[:, None, :, 0] * (py[..., None] - A[:, None, :, 1]) - D[:, None, :, 1] * (px[..., None] - A[:, None, :, 0])
    # a start point A of the area-flipped edge lies on the edge line either way
    L = np.sqrt((D ** 2).sum(-1))[:, None, :]
    d = w / L
    strict = ((w > 0) | ((w == 0) & own[:, None, :])).all(-1)
    near = (d > -margin).all(-1) & (np.abs(d) < margin).any(-1)
    s = w.sum(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        iz = (w[..., 1] / P[:, None, 0, 2] + w[..., 2] / P[:, None, 1, 2] + w[..., 0] / P[:, None, 2, 2]) / s
        z = 1.0 / iz
    return strict, near, z, w


class _Top2:
    """per-pixel nearest (z, id) and second-nearest z over streamed fragments, plus the nearest near-edge z."""

    def __init__(self, n):
        self.z1 = np.full(n, np.inf)
        self.id1 = np.full(n, -1, np.int64)
        self.z2 = np.full(n, np.inf)
        self.zn = np.full(n, np.inf)

    def add(self, pix, z, ids, strict, near):
        if near.any():
            np.minimum.at(self.zn, pix[near], np.where(np.isfinite(z[near]), z[near], -np.inf))
        pix, z, ids = pix[strict], z[strict], ids[strict]
        if not len(pix):
            return
        o = np.lexsort((ids, z, pix))
        pix, z, ids = pix[o], z[o], ids[o]
        first = np.ones(len(pix), bool)
        first[1:] = pix[1:] != pix[:-1]
        fi = np.nonzero(first)[0]
        up, bz1, bid1 = pix[fi], z[fi], ids[fi]
        nxt = fi + 1
        has2 = np.zeros(len(fi), bool)
        has2[nxt < len(pix)] = ~first[nxt[nxt < len(pix)]]
        bz2 = np.where(has2, z[np.minimum(nxt, len(pix) - 1)], np.inf)
        cz1, cid1, cz2 = self.z1[up], self.id1[up], self.z2[up]
        cur_wins = (cz1 < bz1) | ((cz1 == bz1) & (cid1 >= 0) & (cid1 < bid1))
        self.z1[up] = np.where(cur_wins, cz1, bz1)
        self.id1[up] = np.where(cur_wins, cid1, bid1)
        self.z2[up] = np.where(cur_wins, np.minimum(cz2, bz1), np.minimum(cz1, bz2))


def rasterize_image(S, faces, mesh_ids, H, W, znear=0.01, zfar=1e4, F=None):
    """S: screen (u, v, z) [M, V, 3] fp64 of the meshes drawn into this image, mesh_ids [M] their indices in the call.
    Returns (z, id = mesh * F + face, z2, ambiguous), each [H * W]."""
    Fi = np.asarray(faces, np.int64)
    F = len(Fi) if F is None else F
    margin = MARGIN_REL * max(H, W)
    top = _Top2(H * W)
    for m, b in enumerate(mesh_ids):
        P = S[m][Fi]                                                            # [F, 3, 3]
        ok = np.isfinite(P).all((1, 2)) & (P[:, :, 2] > znear).all(1) & ~(P[:, :, 2] > zfar).all(1)
        ok &= (Fi[:, 0] != Fi[:, 1]) & (Fi[:, 1] != Fi[:, 2]) & (Fi[:, 0] != Fi[:, 2])
        fidx = np.nonzero(ok)[0]
        P = P[fidx]
        A, D, own, area = _edges(P)
        keep = area != 0
        fidx, P, A, D, own = fidx[keep], P[keep], A[keep], D[keep], own[keep]
        lo, hi = P[:, :, :2].min(1) - margin, P[:, :, :2].max(1) + margin
        j0 = np.clip(np.ceil(lo[:, 0] - 0.5), 0, W).astype(np.int64)
        j1 = np.clip(np.floor(hi[:, 0] - 0.5), -1, W - 1).astype(np.int64)
        i0 = np.clip(np.ceil(lo[:, 1] - 0.5), 0, H).astype(np.int64)
        i1 = np.clip(np.floor(hi[:, 1] - 0.5), -1, H - 1).astype(np.int64)
        vis = (j0 <= j1) & (i0 <= i1)
        ext = np.maximum(j1 - j0, i1 - i0) + 1
        ids_all = b * F + fidx
        lo_s = 0
        for st_size in [SMALL * 2 ** k for k in range(32)]:
            sel = np.nonzero(vis & (ext > lo_s) & (ext <= st_size))[0]
            lo_s = st_size
            if len(sel):
                dj, di = np.meshgrid(np.arange(st_size), np.arange(st_size))
                dj, di = dj.reshape(-1), di.reshape(-1)
                chunk = max(1, 2_000_000 // (st_size * st_size))
                for c0 in range(0, len(sel), chunk):
                    sl = sel[c0:c0 + chunk]
                    jj, ii = j0[sl, None] + dj, i0[sl, None] + di
                    inb = (jj <= j1[sl, None]) & (ii <= i1[sl, None])
                    st, nr, z, _ = _eval(P[sl], A[sl], D[sl], own[sl], jj + 0.5, ii + 0.5, margin)
                    st &= inb
                    nr &= inb
                    pix = ii * W + jj
                    top.add(pix[inb], z[inb], np.broadcast_to(ids_all[sl, None], pix.shape)[inb], st[inb], nr[inb])
            if st_size >= max(H, W):
                break
    amb = (np.isfinite(top.zn) & (top.zn <= top.z1 * (1 + DEPTH_REL))) | (np.isfinite(top.z2) & (top.z2 <= top.z1 * (1 + DEPTH_REL)))
    return top.z1, top.id1, top.z2, amb


def vertex_normals(cam, faces):
    """unit camera-frame face normals [M, F, 3] and the normalised sums around each vertex [M, V, 3] (zero where undefined)."""
    Fi = np.asarray(faces, np.int64)
    P = cam[:, Fi]
    n = np.cross(P[:, :, 1] - P[:, :, 0], P[:, :, 2] - P[:, :, 0])
    ln = np.linalg.norm(n, axis=-1, keepdims=True)
    fn = np.where(ln > 0, n / np.where(ln > 0, ln, 1), 0)
    vn = np.zeros_like(cam)
    for k in range(3):
        for m in range(cam.shape[0]):
            np.add.at(vn[m], Fi[:, k], fn[m])
    lv = np.linalg.norm(vn, axis=-1, keepdims=True)
    return fn, np.where(lv > 0, vn / np.where(lv > 0, lv, 1), 0)


def render(vertices, faces, intrinsics, H, W, transforms=None, image_of_mesh=None, base_color=(1, 1, 1), lights=(), ambient=0.0,
           smooth=False, znear=0.01, zfar=1e4):
    """The whole call in fp64: dict of face_id, mesh_id, depth [N, H, W], rgb255 (unrounded 255 c) [N, H, W, 3], ambiguous [N, H, W]."""
    v = np.asarray(vertices, np.float32)
    B, V = v.shape[:2]
    Fi = np.asarray(faces, np.int64)
    F = len(Fi)
    img = np.arange(B) if image_of_mesh is None else np.asarray(image_of_mesh, np.int64)
    K = np.asarray(intrinsics, np.float64).reshape(-1, 4)
    N = B if image_of_mesh is None else len(K)
    T = np.broadcast_to(np.eye(3, 4), (B, 3, 4)) if transforms is None else np.asarray(transforms)
    cam, S = project(v, T, K[img])
    col = np.broadcast_to(np.asarray(base_color, np.float64), (B, 3))
    Ls = np.asarray(lights, np.float64).reshape(-1, 7)
    amb = np.broadcast_to(np.asarray(ambient, np.float64), (3,))
    fn, vn = vertex_normals(cam, Fi) if smooth else (None, None)
    out = {k: [] for k in ("face_id", "mesh_id", "depth", "rgb255", "ambiguous", "covered")}
    for n in range(N):
        ms = np.nonzero(img == n)[0]
        z1, id1, z2, a = rasterize_image(S[ms], Fi, ms, H, W, znear, zfar, F)
        cov = id1 >= 0
        b, f = np.where(cov, id1 // F, -1), np.where(cov, id1 % F, -1)
        rgb = np.zeros((H * W, 3))
        pc = np.nonzero(cov)[0]
        if len(pc):
            bb, ff = b[pc], f[pc]
            px, py = pc % W + 0.5, pc // W + 0.5
            z = z1[pc]
            Kn = K[n]
            Pt = np.stack([(px - Kn[2]) / Kn[0] * z, (py - Kn[3]) / Kn[1] * z, z], -1)
            C = cam[bb[:, None], Fi[ff]]                                         # [k, 3, 3]
            nrm = np.cross(C[:, 1] - C[:, 0], C[:, 2] - C[:, 0])
            if smooth:
                Sp = S[bb[:, None], Fi[ff]]
                A, D, own, _ = _edges(Sp)
                w = D[:, :, 0] * (py[:, None] - A[:, :, 1]) - D[:, :, 1] * (px[:, None] - A[:, :, 0])
                s = w.sum(-1)
                mu = np.stack([w[:, 1] / Sp[:, 0, 2], w[:, 2] / Sp[:, 1, 2], w[:, 0] / Sp[:, 2, 2]], -1) / s[:, None] * z[:, None]
                vv = vn[bb[:, None], Fi[ff]]
                sm = (mu[:, :, None] * vv).sum(1)
                nrm = np.where((np.linalg.norm(sm, axis=-1) > 0)[:, None], sm, nrm)
            nrm = nrm / np.linalg.norm(nrm, axis=-1, keepdims=True)
            nrm = np.where(((nrm * Pt).sum(-1) > 0)[:, None], -nrm, nrm)
            lit = np.broadcast_to(amb, (len(pc), 3)).copy()
            for L in Ls:
                d = np.broadcast_to(L[1:4], Pt.shape) if L[0] == 0 else L[1:4] - Pt
                d = d / np.linalg.norm(d, axis=-1, keepdims=True)
                lit += L[4:7] * np.maximum(0, (nrm * d).sum(-1))[:, None]
            rgb[pc] = 255 * np.clip(col[bb] * lit, 0, 1)
        out["face_id"].append(f.reshape(H, W))
        out["mesh_id"].append(b.reshape(H, W))
        out["depth"].append(np.where(cov, z1, 0).reshape(H, W))
        out["rgb255"].append(rgb.reshape(H, W, 3))
        out["ambiguous"].append(a.reshape(H, W))
        out["covered"].append(cov.reshape(H, W))
    return {k: np.stack(x) for k, x in out.items()}


def body_torus(n_u=84, n_v=82, seed=3):
    """A closed deformed torus of body size (about 1.7 m tall, standing along y): F = 2 n_u n_v."""
    import si_ref
    X, F = si_ref.torus(n_u=n_u, n_v=n_v, R=0.6, r=0.25)
    X = si_ref.smooth_deform(X, seed, amp=0.05)
    X = X * np.array([0.8, 1.0, 1.0], np.float32)                           # ring in the x-y plane: a 1.7 m tall loop
    return X.astype(np.float32), F


def decode_png(data):
    """uint8 [H, W, 3] of an 8-bit RGB PNG with filter 0 on every row (what dposer_amd.body_model.visual.encode_png writes)."""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat = 8, b""
    w = h = None
    while pos < len(data):
        (n,) = struct.unpack(">I", data[pos:pos + 4])
        kind, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        (crc,) = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        assert crc == zlib.crc32(kind + body) & 0xFFFFFFFF
        if kind == b"IHDR":
            w, h, depth, ctype = struct.unpack(">IIBB", body[:10])
            assert (depth, ctype) == (8, 2)
        elif kind == b"IDAT":
            idat += body
        pos += 12 + n
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + 3 * w)
    assert (raw[:, 0] == 0).all()
    return raw[:, 1:].reshape(h, w, 3)
