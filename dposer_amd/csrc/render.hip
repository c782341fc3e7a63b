// dposer_render_meshes -- the mesh renderer of lib/body_model/visual.py:132-366 (pyrender / pytorch3d there): B meshes sharing one face
// list, rasterised with a depth test into num_images images.  The rules are the header's (include/dposer_hip.h); all fp32.
//
//   k_rd_vertices      one lane per (mesh, vertex): camera-frame position and projected (u, v, z), once per vertex.
//   k_rd_face_normals  (smooth) one lane per (mesh, face): unit camera-frame face normal.
//   k_rd_vertex_normals(smooth) one lane per (mesh, vertex): normalised sum over the vertex -> face CSR (its order: deterministic).
//   k_rd_bin<pass>     one lane per (mesh, face): the box of pixel centres it can cover.  A face touching at most kMaxTiles tiles of
//                      kTile x kTile pixels goes on those tiles' lists, a larger one on its image's large list.  Pass 0 counts, pass 1
//                      fills through cursors from k_rd_scan (the order inside a list is the atomics' and does not matter: min key).
//   k_rd_raster        one workgroup per (image, tile): the tile's z-buffer of 64-bit keys in LDS; its own list one lane per face, the
//                      large list staged 256 faces at a time and swept one lane per 4 pixels; then every pixel of the tile is shaded and
//                      written exactly once.  No global atomics on the fragment path.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "common.h"

namespace {

constexpr int kTile = 32;                 // tile edge in pixels
constexpr int kMaxTiles = 4;              // faces touching more tiles go on the image's large list
constexpr int kThreads = 256;             // raster workgroup; kTile * kTile / kThreads pixels per lane
constexpr int kPixPerLane = kTile * kTile / kThreads;
constexpr uint64_t kEmpty = ~0ull;

struct F3 { float x, y, z; };

// a face ready to rasterise: edges in winding order (e0 = v0 -> v1, e1 = v1 -> v2, e2 = v2 -> v0), each stored canonically
struct Tri {
    float xl[3], yl[3], dx[3], dy[3];    // lower-index endpoint and (higher - lower) of each edge
    float iz[3];                          // 1 / z of the corners
    int bits;                             // bit e: negate edge e;  bit 3 + e: edge e owns an exact zero (top-left)
    int j0, j1, i0, i1;                   // inclusive pixel box (clipped to the image)
    uint32_t id;                          // b * F + f
};

__device__ __forceinline__ bool finite3(float4 p) { return isfinite(p.x) && isfinite(p.y) && isfinite(p.z); }

// false: the face is dropped or covers no pixel centre
__device__ bool tri_setup(const float4* __restrict__ scr, const int32_t* __restrict__ faces, int32_t V, int32_t F, uint32_t id, int H, int W,
                          float znear, float zfar, Tri& t) {
    const uint32_t b = id / (uint32_t)F, f = id - b * (uint32_t)F;
    const int idx[3] = {faces[(int64_t)f * 3], faces[(int64_t)f * 3 + 1], faces[(int64_t)f * 3 + 2]};
    if (idx[0] == idx[1] || idx[1] == idx[2] || idx[0] == idx[2]) return false;
    const float4* sb = scr + (int64_t)b * V;
    const float4 p[3] = {sb[idx[0]], sb[idx[1]], sb[idx[2]]};
    if (!finite3(p[0]) || !finite3(p[1]) || !finite3(p[2])) return false;
    if (p[0].z <= znear || p[1].z <= znear || p[2].z <= znear) return false;
    if (p[0].z > zfar && p[1].z > zfar && p[2].z > zfar) return false;
    const float area = (p[1].x - p[0].x) * (p[2].y - p[0].y) - (p[1].y - p[0].y) * (p[2].x - p[0].x);
    if (!(area != 0.f) || !isfinite(area)) return false;
    int bits = 0;
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        const int a = e, c = e == 2 ? 0 : e + 1;
        const bool fwd = idx[a] < idx[c];
        const float4 lo = fwd ? p[a] : p[c], hi = fwd ? p[c] : p[a];
        t.xl[e] = lo.x; t.yl[e] = lo.y;
        t.dx[e] = hi.x - lo.x; t.dy[e] = hi.y - lo.y;
        const bool neg = fwd != (area > 0.f);             // oriented value = -canonical when exactly one of (reversed, negative area)
        const float ox = neg ? -t.dx[e] : t.dx[e], oy = neg ? -t.dy[e] : t.dy[e];
        bits |= (neg ? 1 : 0) << e;
        bits |= ((oy < 0.f || (oy == 0.f && ox > 0.f)) ? 1 : 0) << (3 + e);
        t.iz[e] = 1.0f / p[e].z;
    }
    t.bits = bits;
    const float umin = fminf(p[0].x, fminf(p[1].x, p[2].x)), umax = fmaxf(p[0].x, fmaxf(p[1].x, p[2].x));
    const float vmin = fminf(p[0].y, fminf(p[1].y, p[2].y)), vmax = fmaxf(p[0].y, fmaxf(p[1].y, p[2].y));
    // centres j + 0.5 in [umin, umax]; clamp before converting (corners near znear project far away)
    t.j0 = (int)ceilf(fminf(fmaxf(umin - 0.5f, -1.f), (float)W));
    t.j1 = (int)floorf(fminf(fmaxf(umax - 0.5f, -1.f), (float)W));
    t.i0 = (int)ceilf(fminf(fmaxf(vmin - 0.5f, -1.f), (float)H));
    t.i1 = (int)floorf(fminf(fmaxf(vmax - 0.5f, -1.f), (float)H));
    t.j0 = max(t.j0, 0); t.j1 = min(t.j1, W - 1);
    t.i0 = max(t.i0, 0); t.i1 = min(t.i1, H - 1);
    t.id = id;
    return t.j0 <= t.j1 && t.i0 <= t.i1;
}

// oriented edge values at (px, py); true when the centre is covered
__device__ __forceinline__ bool tri_cover(const Tri& t, float px, float py, float (&w)[3]) {
    bool in = true;
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        const float c = t.dx[e] * (py - t.yl[e]) - t.dy[e] * (px - t.xl[e]);
        w[e] = ((t.bits >> e) & 1) ? -c : c;
        in = in && (w[e] > 0.f || (w[e] == 0.f && ((t.bits >> (3 + e)) & 1)));
    }
    return in;
}

// 1 / z at the covered centre: the edge opposite corner k is e = k + 1 (mod 3)
__device__ __forceinline__ float tri_depth(const Tri& t, const float (&w)[3]) {
    const float s = w[0] + w[1] + w[2];
    const float iz = (w[1] * t.iz[0] + w[2] * t.iz[1] + w[0] * t.iz[2]) / s;
    return 1.0f / iz;
}

__device__ __forceinline__ uint64_t frag_key(float z, uint32_t id) { return ((uint64_t)__float_as_uint(z) << 32) | id; }

__global__ void __launch_bounds__(256) k_rd_vertices(const float* __restrict__ verts, int64_t n, int32_t V, const float* __restrict__ xf,
                                                     const int32_t* __restrict__ image_of_mesh, const float* __restrict__ intr,
                                                     float4* __restrict__ cam, float4* __restrict__ scr) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const int64_t b = k / V;
    const float* p = verts + k * 3;
    const float x = p[0], y = p[1], z = p[2];
    const float* T = xf + b * 12;
    const float cx = T[0] * x + T[1] * y + T[2] * z + T[3];
    const float cy = T[4] * x + T[5] * y + T[6] * z + T[7];
    const float cz = T[8] * x + T[9] * y + T[10] * z + T[11];
    const int64_t img = image_of_mesh ? (int64_t)image_of_mesh[b] : b;
    const float4 K = reinterpret_cast<const float4*>(intr)[img];
    cam[k] = float4{cx, cy, cz, 0.f};
    scr[k] = float4{K.x * cx / cz + K.z, K.y * cy / cz + K.w, cz, 0.f};
}

__device__ __forceinline__ F3 unit_or_zero(F3 v) {
    const float l = sqrtf(v.x * v.x + v.y * v.y + v.z * v.z);
    if (!(l > 0.f) || !isfinite(l)) return {0.f, 0.f, 0.f};
    return {v.x / l, v.y / l, v.z / l};
}

__device__ __forceinline__ F3 face_normal(const float4* __restrict__ cb, const int32_t* __restrict__ faces, int64_t f) {
    const float4 a = cb[faces[f * 3]], b = cb[faces[f * 3 + 1]], c = cb[faces[f * 3 + 2]];
    const float ux = b.x - a.x, uy = b.y - a.y, uz = b.z - a.z, vx = c.x - a.x, vy = c.y - a.y, vz = c.z - a.z;
    return unit_or_zero({uy * vz - uz * vy, uz * vx - ux * vz, ux * vy - uy * vx});
}

__global__ void __launch_bounds__(256) k_rd_face_normals(const float4* __restrict__ cam, int32_t V, const int32_t* __restrict__ faces,
                                                         int32_t F, int64_t n, float4* __restrict__ fn) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const int64_t b = k / F;
    const F3 u = face_normal(cam + b * V, faces, k - b * F);
    fn[k] = float4{u.x, u.y, u.z, 0.f};
}

__global__ void __launch_bounds__(256) k_rd_vertex_normals(const float4* __restrict__ fn, int32_t F, int32_t V, const int32_t* __restrict__ vf_ptr,
                                                           const int32_t* __restrict__ vf_face, int64_t n, float4* __restrict__ vn) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const int64_t b = k / V;
    const int v = (int)(k - b * V);
    const float4* fb = fn + b * F;
    F3 s = {0.f, 0.f, 0.f};
    for (int e = vf_ptr[v]; e < vf_ptr[v + 1]; ++e) {
        const float4 q = fb[vf_face[e]];
        s.x += q.x; s.y += q.y; s.z += q.z;
    }
    const F3 u = unit_or_zero(s);
    vn[k] = float4{u.x, u.y, u.z, 0.f};
}

struct BinGeom {
    int tiles_x, tiles_per_image;
    int64_t n_tiles;                      // num_images * tiles_per_image; bin n_tiles + image = the image's large list
};

template <int kPass>
__global__ void __launch_bounds__(256) k_rd_bin(const float4* __restrict__ scr, const int32_t* __restrict__ faces, int32_t V, int32_t F,
                                                int64_t n, const int32_t* __restrict__ image_of_mesh, int H, int W, float znear, float zfar,
                                                BinGeom g, uint32_t* __restrict__ counts, uint32_t* __restrict__ cursor,
                                                uint32_t* __restrict__ entries) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    Tri t;
    if (!tri_setup(scr, faces, V, F, (uint32_t)k, H, W, znear, zfar, t)) return;
    const int64_t b = k / F;
    const int64_t img = image_of_mesh ? (int64_t)image_of_mesh[b] : b;
    const int tx0 = t.j0 / kTile, tx1 = t.j1 / kTile, ty0 = t.i0 / kTile, ty1 = t.i1 / kTile;
    const int64_t base = img * g.tiles_per_image;
    if ((tx1 - tx0 + 1) * (ty1 - ty0 + 1) <= kMaxTiles) {
        for (int ty = ty0; ty <= ty1; ++ty)
            for (int tx = tx0; tx <= tx1; ++tx) {
                const int64_t bin = base + ty * g.tiles_x + tx;
                if (kPass == 0) atomicAdd(&counts[bin], 1u);
                else entries[atomicAdd(&cursor[bin], 1u)] = (uint32_t)k;
            }
    } else {
        const int64_t bin = g.n_tiles + img;
        if (kPass == 0) atomicAdd(&counts[bin], 1u);
        else entries[atomicAdd(&cursor[bin], 1u)] = (uint32_t)k;
    }
}

// exclusive scan of counts[0, n) into offsets (and the fill cursors), one workgroup: each lane scans a contiguous chunk serially
__global__ void __launch_bounds__(1024) k_rd_scan(const uint32_t* __restrict__ counts, int64_t n, uint32_t* __restrict__ offsets,
                                                  uint32_t* __restrict__ cursor) {
    __shared__ uint32_t s_part[1024];
    const int tid = threadIdx.x;
    const int64_t chunk = (n + 1023) / 1024;
    const int64_t lo = min(n, tid * chunk), hi = min(n, lo + chunk);
    uint32_t sum = 0;
    for (int64_t i = lo; i < hi; ++i) sum += counts[i];
    s_part[tid] = sum;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {                // Hillis-Steele inclusive scan of the chunk sums
        const uint32_t v = tid >= d ? s_part[tid - d] : 0u;
        __syncthreads();
        s_part[tid] += v;
        __syncthreads();
    }
    uint32_t run = s_part[tid] - sum;
    for (int64_t i = lo; i < hi; ++i) {
        offsets[i] = run;
        cursor[i] = run;
        run += counts[i];
    }
}

struct ShadeArgs {
    const float4* cam;
    const float4* vn;                     // smooth only
    const int32_t* faces;
    const float* base_color;
    const float* lights;
    int32_t num_lights;
    float amb[3];
    int32_t smooth;
    const uint8_t* background;
    int64_t background_stride;
    uint8_t bg_color[4];
};

__device__ __forceinline__ uint8_t to_u8(float c) { return (uint8_t)rintf(255.0f * fminf(fmaxf(c, 0.f), 1.f)); }

__global__ void __launch_bounds__(kThreads) k_rd_raster(const float4* __restrict__ scr, const int32_t* __restrict__ faces, int32_t V, int32_t F,
                                                        int H, int W, const float* __restrict__ intr, float znear, float zfar, BinGeom g,
                                                        const uint32_t* __restrict__ counts, const uint32_t* __restrict__ offsets,
                                                        const uint32_t* __restrict__ entries, ShadeArgs sa, uint8_t* __restrict__ rgb,
                                                        float* __restrict__ depth, int32_t* __restrict__ face_id, int32_t* __restrict__ mesh_id) {
    __shared__ uint64_t s_key[kTile * kTile];
    __shared__ Tri s_tri[kThreads];
    __shared__ int s_ok[kThreads];
    const int tid = threadIdx.x;
    const int64_t tile = blockIdx.x;
    const int64_t img = tile / g.tiles_per_image;
    const int tl = (int)(tile - img * g.tiles_per_image);
    const int ty = tl / g.tiles_x, tx = tl - ty * g.tiles_x;
    const int pj0 = tx * kTile, pi0 = ty * kTile;
    const int pj1 = min(pj0 + kTile, W) - 1, pi1 = min(pi0 + kTile, H) - 1;
#pragma unroll
    for (int q = 0; q < kPixPerLane; ++q) s_key[tid + q * kThreads] = kEmpty;
    __syncthreads();

    // the tile's own list: one lane per face over its box inside the tile
    {
        const uint32_t o = offsets[tile], c = counts[tile];
        for (uint32_t e = tid; e < c; e += kThreads) {
            Tri t;
            if (!tri_setup(scr, faces, V, F, entries[o + e], H, W, znear, zfar, t)) continue;
            const int j0 = max(t.j0, pj0), j1 = min(t.j1, pj1), i0 = max(t.i0, pi0), i1 = min(t.i1, pi1);
            for (int i = i0; i <= i1; ++i)
                for (int j = j0; j <= j1; ++j) {
                    float w[3];
                    if (tri_cover(t, (float)j + 0.5f, (float)i + 0.5f, w))
                        atomicMin((unsigned long long*)&s_key[(i - pi0) * kTile + (j - pj0)], (unsigned long long)frag_key(tri_depth(t, w), t.id));
                }
        }
    }
    // the image's large list: 256 faces staged at a time, each swept by the whole workgroup
    {
        const int64_t lb = g.n_tiles + img;
        const uint32_t o = offsets[lb], c = counts[lb];
        for (uint32_t e0 = 0; e0 < c; e0 += kThreads) {
            Tri t;
            bool ok = false;
            if (e0 + tid < c && tri_setup(scr, faces, V, F, entries[o + e0 + tid], H, W, znear, zfar, t))
                ok = t.j0 <= pj1 && t.j1 >= pj0 && t.i0 <= pi1 && t.i1 >= pi0;
            if (ok) s_tri[tid] = t;
            s_ok[tid] = ok;
            __syncthreads();
            const int n = (int)min((uint32_t)kThreads, c - e0);
            for (int s = 0; s < n; ++s) {
                if (!s_ok[s]) continue;
                const Tri& ts = s_tri[s];
#pragma unroll
                for (int q = 0; q < kPixPerLane; ++q) {
                    const int p = tid + q * kThreads;
                    const int i = pi0 + (p >> 5), j = pj0 + (p & (kTile - 1));
                    if (i < ts.i0 || i > ts.i1 || j < ts.j0 || j > ts.j1) continue;
                    float w[3];
                    if (tri_cover(ts, (float)j + 0.5f, (float)i + 0.5f, w))
                        atomicMin((unsigned long long*)&s_key[p], (unsigned long long)frag_key(tri_depth(ts, w), ts.id));
                }
            }
            __syncthreads();                               // (the next chunk overwrites the staged faces)
        }
    }
    __syncthreads();

    // resolve: shade and write every pixel of the tile once
    const float4 K = reinterpret_cast<const float4*>(intr)[img];
#pragma unroll
    for (int q = 0; q < kPixPerLane; ++q) {
        const int p = tid + q * kThreads;
        const int i = pi0 + (p >> 5), j = pj0 + (p & (kTile - 1));
        if (i >= H || j >= W) continue;
        const int64_t pix = (img * H + i) * (int64_t)W + j;
        const uint64_t key = s_key[p];
        float zout = 0.f;
        int32_t fid = -1, mid = -1;
        uint8_t out[3];
        if (key == kEmpty) {
            const uint8_t* bg = sa.background ? sa.background + img * sa.background_stride + ((int64_t)i * W + j) * 3 : sa.bg_color;
            out[0] = bg[0]; out[1] = bg[1]; out[2] = bg[2];
        } else {
            const uint32_t id = (uint32_t)key;
            const uint32_t b = id / (uint32_t)F, f = id - b * (uint32_t)F;
            const float z = __uint_as_float((uint32_t)(key >> 32));
            zout = z;
            fid = (int32_t)f;
            mid = (int32_t)b;
            const float px = (float)j + 0.5f, py = (float)i + 0.5f;
            const F3 P = {(px - K.z) / K.x * z, (py - K.w) / K.y * z, z};
            const float4* cb = sa.cam + (int64_t)b * V;
            F3 n;
            if (sa.smooth) {
                Tri t;
                tri_setup(scr, faces, V, F, id, H, W, znear, zfar, t);
                float w[3];
                tri_cover(t, px, py, w);
                // perspective-correct weights of the corners: (b_k / z_k) * z
                const float s = w[0] + w[1] + w[2];
                const float m0 = w[1] / s * t.iz[0] * z, m1 = w[2] / s * t.iz[1] * z, m2 = w[0] / s * t.iz[2] * z;
                const float4* nb = sa.vn + (int64_t)b * V;
                const float4 n0 = nb[faces[(int64_t)f * 3]], n1 = nb[faces[(int64_t)f * 3 + 1]], n2 = nb[faces[(int64_t)f * 3 + 2]];
                n = unit_or_zero({m0 * n0.x + m1 * n1.x + m2 * n2.x, m0 * n0.y + m1 * n1.y + m2 * n2.y, m0 * n0.z + m1 * n1.z + m2 * n2.z});
                if (n.x == 0.f && n.y == 0.f && n.z == 0.f) n = face_normal(cb, faces, f);
            } else {
                n = face_normal(cb, faces, f);
            }
            if (n.x * P.x + n.y * P.y + n.z * P.z > 0.f) n = {-n.x, -n.y, -n.z};      // face the camera (view vector -P)
            float lit[3] = {sa.amb[0], sa.amb[1], sa.amb[2]};
            for (int l = 0; l < sa.num_lights; ++l) {
                const float* L = sa.lights + l * 7;
                F3 d = {L[1], L[2], L[3]};
                if (L[0] != 0.f) d = {L[1] - P.x, L[2] - P.y, L[3] - P.z};
                d = unit_or_zero(d);
                const float c = fmaxf(0.f, n.x * d.x + n.y * d.y + n.z * d.z);
                lit[0] += L[4] * c; lit[1] += L[5] * c; lit[2] += L[6] * c;
            }
            const float* bc = sa.base_color + (int64_t)b * 3;
            out[0] = to_u8(bc[0] * lit[0]); out[1] = to_u8(bc[1] * lit[1]); out[2] = to_u8(bc[2] * lit[2]);
        }
        if (rgb) { rgb[pix * 3] = out[0]; rgb[pix * 3 + 1] = out[1]; rgb[pix * 3 + 2] = out[2]; }
        if (depth) depth[pix] = zout;
        if (face_id) face_id[pix] = fid;
        if (mesh_id) mesh_id[pix] = mid;
    }
}

struct Layout {
    int64_t cam, scr, fn, vn, counts, offsets, cursor, entries, total;
};

Layout layout(int64_t B, int32_t V, int32_t F, int64_t N, int32_t H, int32_t W) {
    const int64_t tiles = N * ceil_div(H, kTile) * ceil_div(W, kTile), bins = tiles + N;
    Layout l;
    int64_t o = 0;
    auto take = [&](int64_t bytes) { const int64_t at = o; o += round_up(bytes, 256); return at; };
    l.cam = take(B * V * 16);
    l.scr = take(B * V * 16);
    l.fn = take(B * F * 16);
    l.vn = take(B * V * 16);
    l.counts = take(bins * 4);
    l.offsets = take(bins * 4);
    l.cursor = take(bins * 4);
    l.entries = take((int64_t)(kMaxTiles + 1) * B * F * 4);   // at most kMaxTiles tile entries or one large-list entry per face
    l.total = o;
    return l;
}

}  // namespace

extern "C" int64_t dposer_render_scratch_bytes(int64_t num_meshes, int32_t num_vertices, int32_t num_faces, int64_t num_images, int32_t height,
                                               int32_t width) {
    if (num_meshes < 0 || num_vertices <= 0 || num_faces <= 0 || num_images <= 0 || height <= 0 || width <= 0) return 0;
    return layout(num_meshes > 0 ? num_meshes : 1, num_vertices, num_faces, num_images, height, width).total;
}

extern "C" int dposer_render_meshes(const dposer_render_args* a, void* stream) {
    DP_RANGE();
    DP_CHECK_ARG(a != nullptr, "args is NULL");
    DP_CHECK_ARG(a->num_meshes >= 0 && a->num_images >= 0, "num_meshes and num_images must be >= 0");
    DP_CHECK_ARG(a->num_vertices > 0 && a->num_faces > 0, "num_vertices and num_faces must be > 0");
    DP_CHECK_ARG(a->height > 0 && a->width > 0, "height and width must be > 0");
    if (a->num_images == 0) return DPOSER_OK;
    DP_CHECK_ARG(a->image_of_mesh != nullptr || a->num_meshes == a->num_images, "without image_of_mesh, num_meshes must equal num_images");
    DP_CHECK_ARG(a->intrinsics && a->scratch, "intrinsics and scratch are required");
    DP_CHECK_ARG(((uintptr_t)a->scratch & 255) == 0, "scratch must be 256-byte aligned");
    DP_CHECK_ARG(a->znear > 0.f && a->zfar > a->znear, "need 0 < znear < zfar");
    DP_CHECK_ARG(a->num_lights >= 0 && (a->num_lights == 0 || a->lights), "lights is NULL");
    const int64_t B = a->num_meshes, N = a->num_images;
    const int32_t V = a->num_vertices, F = a->num_faces, H = a->height, W = a->width;
    DP_CHECK_ARG(B * F < (int64_t)UINT32_MAX, "num_meshes x num_faces must stay below 2^32 - 1 (split the call)");
    const int tiles_x = (int)ceil_div(W, kTile), tiles_y = (int)ceil_div(H, kTile);
    const int64_t n_tiles = N * tiles_x * tiles_y;
    DP_CHECK_ARG(n_tiles <= INT32_MAX, "too many image tiles for one call");
    const Layout l = layout(B > 0 ? B : 1, V, F, N, H, W);
    DP_CHECK_ARG((int64_t)(kMaxTiles + 1) * B * F <= UINT32_MAX, "num_meshes x num_faces too large for 32-bit list offsets (split the call)");
    hipStream_t st = (hipStream_t)stream;
    char* s = (char*)a->scratch;
    float4* cam = (float4*)(s + l.cam);
    float4* scr = (float4*)(s + l.scr);
    float4* fn = (float4*)(s + l.fn);
    float4* vn = (float4*)(s + l.vn);
    uint32_t* counts = (uint32_t*)(s + l.counts);
    uint32_t* offsets = (uint32_t*)(s + l.offsets);
    uint32_t* cursor = (uint32_t*)(s + l.cursor);
    uint32_t* entries = (uint32_t*)(s + l.entries);
    const BinGeom g = {tiles_x, tiles_x * tiles_y, n_tiles};
    const int64_t bins = n_tiles + N;

    DP_CHECK_HIP(hipMemsetAsync(counts, 0, bins * 4, st));
    if (B > 0) {
        DP_CHECK_ARG(a->vertices && a->faces && a->transforms && a->base_color, "vertices, faces, transforms and base_color are required");
        DP_CHECK_ARG(!a->smooth || (a->vf_ptr && a->vf_face), "smooth shading needs vf_ptr and vf_face");
        const int64_t nv = B * V, nf = B * F;
        hipLaunchKernelGGL(k_rd_vertices, dim3((unsigned)ceil_div(nv, 256)), dim3(256), 0, st, a->vertices, nv, V, a->transforms,
                           a->image_of_mesh, a->intrinsics, cam, scr);
        DP_CHECK_LAUNCH();
        if (a->smooth) {
            hipLaunchKernelGGL(k_rd_face_normals, dim3((unsigned)ceil_div(nf, 256)), dim3(256), 0, st, (const float4*)cam, V, a->faces, F, nf, fn);
            DP_CHECK_LAUNCH();
            hipLaunchKernelGGL(k_rd_vertex_normals, dim3((unsigned)ceil_div(nv, 256)), dim3(256), 0, st, (const float4*)fn, F, V, a->vf_ptr,
                               a->vf_face, nv, vn);
            DP_CHECK_LAUNCH();
        }
        hipLaunchKernelGGL(k_rd_bin<0>, dim3((unsigned)ceil_div(nf, 256)), dim3(256), 0, st, (const float4*)scr, a->faces, V, F, nf,
                           a->image_of_mesh, H, W, a->znear, a->zfar, g, counts, cursor, entries);
        DP_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_rd_scan, dim3(1), dim3(1024), 0, st, (const uint32_t*)counts, bins, offsets, cursor);
        DP_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_rd_bin<1>, dim3((unsigned)ceil_div(nf, 256)), dim3(256), 0, st, (const float4*)scr, a->faces, V, F, nf,
                           a->image_of_mesh, H, W, a->znear, a->zfar, g, counts, cursor, entries);
        DP_CHECK_LAUNCH();
    } else {
        DP_CHECK_HIP(hipMemsetAsync(offsets, 0, bins * 4, st));
    }
    ShadeArgs sa;
    sa.cam = cam;
    sa.vn = vn;
    sa.faces = a->faces;
    sa.base_color = a->base_color;
    sa.lights = a->lights;
    sa.num_lights = a->num_lights;
    sa.amb[0] = a->ambient[0]; sa.amb[1] = a->ambient[1]; sa.amb[2] = a->ambient[2];
    sa.smooth = a->smooth;
    sa.background = a->background;
    sa.background_stride = a->background_stride;
    for (int c = 0; c < 4; ++c) sa.bg_color[c] = a->background_color[c];
    hipLaunchKernelGGL(k_rd_raster, dim3((unsigned)n_tiles), dim3(kThreads), 0, st, (const float4*)scr, a->faces, V, F, H, W, a->intrinsics,
                       a->znear, a->zfar, g, (const uint32_t*)counts, (const uint32_t*)offsets, (const uint32_t*)entries, sa, a->rgb, a->depth,
                       a->face_id, a->mesh_id);
    DP_CHECK_LAUNCH();
    return DPOSER_OK;
}
