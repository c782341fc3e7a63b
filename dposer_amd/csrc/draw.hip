// dposer_draw_skeletons -- the skeleton plots of lib/body_model/visual.py:18-119 (one matplotlib 3-D figure per frame there): B frames of
// K bones and J discs in one call.  dposer_compose_panels -- the per-frame numpy / cv2 compositing of lib/utils/motion_video.py:6-55,95-126
// (crop_bottom, cv2.resize, resize_or_crop, add_title, np.hstack): N frames of P panels in one call.  The rules are the header's
// (include/dposer_hip.h); all fp32, no contraction.
//
//   k_dr_prepare   one workgroup per frame: project the joints, build the K + J primitives, rank them by their depth keys (every order
//                  decision of the frame is taken here, once) and write them in paint order.
//   k_dr_paint     one workgroup per (frame, 64 x 16 tile), a lane per four horizontally adjacent pixels: the frame's primitives are
//                  staged 256 at a time, keeping in LDS only those whose padded screen box touches the tile (in order: ballot compaction),
//                  then blended over the background in registers; 12 bytes leave the lane as three dwords.
//   k_cp_compose   a lane per four horizontally adjacent output pixels: panel lookup, placement, crop, optional bilinear tap, strip.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "common.h"

namespace {

constexpr int kTileW = 64, kTileH = 16;   // paint tile in pixels
constexpr int kThreads = 256;             // kTileW / 4 lanes across, kTileH down
constexpr int kLanesX = kTileW / 4;

// a primitive in paint order: segment (ax, ay) - (bx, by) (a disc: a == b), radius r (< 0: dropped), colour
struct Prim {
    float ax, ay, bx, by, r;
    float cr, cg, cb;
};
static_assert(sizeof(Prim) == 32, "Prim is 32 bytes");

struct View {
    float s, X0, Y0, cx, cy;
    int y_up, z_toward_viewer;
};

__device__ __forceinline__ bool finite_joint(const float* p) { return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]); }

__global__ void __launch_bounds__(kThreads) k_dr_prepare(const float* __restrict__ joints, int32_t J, int32_t K, const uint8_t* __restrict__ visible,
                                                         const int32_t* __restrict__ bones, const uint8_t* __restrict__ bone_color,
                                                         const uint8_t* __restrict__ joint_color, View vw, float line_r, float joint_r,
                                                         Prim* __restrict__ sorted) {
    __shared__ float s_key[DPOSER_DRAW_MAX_PRIMITIVES];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int P = K + J;
    const float* jb = joints + b * (int64_t)J * 3;
    Prim* out = sorted + b * (int64_t)P;
    // keys (a dropped primitive keeps a finite key: it is ranked like any other and skipped when painted)
    for (int p = tid; p < P; p += kThreads) {
        float key = 0.f;
        if (p < K) {
            const int j0 = bones[2 * p], j1 = bones[2 * p + 1];
            const float* a = jb + (int64_t)j0 * 3;
            const float* c = jb + (int64_t)j1 * 3;
            if (finite_joint(a) && finite_joint(c)) {
                const float da = vw.z_toward_viewer ? -a[2] : a[2], dc = vw.z_toward_viewer ? -c[2] : c[2];
                key = 0.5f * (da + dc);
            }
        } else {
            const float* a = jb + (int64_t)(p - K) * 3;
            if (finite_joint(a)) key = (vw.z_toward_viewer ? -a[2] : a[2]) - 1e-3f;
        }
        s_key[p] = key;
    }
    __syncthreads();
    for (int p = tid; p < P; p += kThreads) {
        const float key = s_key[p];
        int rank = 0;                                     // primitives painted before p: farther, or as far with a lower index
        for (int q = 0; q < P; ++q) {
            const float kq = s_key[q];
            rank += (kq > key || (kq == key && q < p)) ? 1 : 0;
        }
        Prim pr;
        pr.ax = pr.ay = pr.bx = pr.by = 0.f;
        pr.r = -1.f;
        pr.cr = pr.cg = pr.cb = 0.f;
        int j0, j1;
        const uint8_t* col;
        if (p < K) {
            j0 = bones[2 * p]; j1 = bones[2 * p + 1];
            col = bone_color + (int64_t)p * 3;
        } else {
            j0 = j1 = p - K;
            col = joint_color + (int64_t)(p - K) * 3;
        }
        const float* a = jb + (int64_t)j0 * 3;
        const float* c = jb + (int64_t)j1 * 3;
        const bool vis = !visible || (visible[j0] != 0 && visible[j1] != 0);
        if (vis && finite_joint(a) && finite_joint(c)) {
            pr.ax = vw.cx + vw.s * (a[0] - vw.X0);
            pr.bx = vw.cx + vw.s * (c[0] - vw.X0);
            const float ya = vw.s * (a[1] - vw.Y0), yc = vw.s * (c[1] - vw.Y0);
            pr.ay = vw.y_up ? vw.cy - ya : vw.cy + ya;
            pr.by = vw.y_up ? vw.cy - yc : vw.cy + yc;
            pr.r = p < K ? line_r : joint_r;
            pr.cr = (float)col[0]; pr.cg = (float)col[1]; pr.cb = (float)col[2];
            // a projection that overflowed leaves nothing to draw
            if (!(isfinite(pr.ax) && isfinite(pr.ay) && isfinite(pr.bx) && isfinite(pr.by))) pr.r = -1.f;
        }
        out[rank] = pr;
    }
}

__device__ __forceinline__ float coverage(const Prim& p, float px, float py) {
    const float ex = p.bx - p.ax, ey = p.by - p.ay;
    const float qx = px - p.ax, qy = py - p.ay;
    const float l2 = ex * ex + ey * ey;
    float t = 0.f;
    if (l2 > 0.f) t = fminf(fmaxf((qx * ex + qy * ey) / l2, 0.f), 1.f);
    const float dx = qx - t * ex, dy = qy - t * ey;
    const float d = sqrtf(dx * dx + dy * dy);
    return fminf(fmaxf(p.r + 0.5f - d, 0.f), 1.f);
}

struct Dw3 { uint32_t a, b, c; };

__device__ __forceinline__ void load12(const uint8_t* p, bool dwords, uint8_t (&v)[12]) {
    if (dwords) {
        const Dw3 w = *reinterpret_cast<const Dw3*>(p);
        const uint32_t u[3] = {w.a, w.b, w.c};
#pragma unroll
        for (int i = 0; i < 12; ++i) v[i] = (uint8_t)(u[i >> 2] >> (8 * (i & 3)));
    } else {
#pragma unroll
        for (int i = 0; i < 12; ++i) v[i] = p[i];
    }
}

__device__ __forceinline__ void store12(uint8_t* p, const uint8_t (&v)[12]) {
    Dw3 w;
    w.a = (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16) | ((uint32_t)v[3] << 24);
    w.b = (uint32_t)v[4] | ((uint32_t)v[5] << 8) | ((uint32_t)v[6] << 16) | ((uint32_t)v[7] << 24);
    w.c = (uint32_t)v[8] | ((uint32_t)v[9] << 8) | ((uint32_t)v[10] << 16) | ((uint32_t)v[11] << 24);
    *reinterpret_cast<Dw3*>(p) = w;
}

// kDwords: width % 4 == 0 and every base pointer / stride is a multiple of 4, so the 12 bytes of a lane are three aligned dwords
template <bool kDwords>
__global__ void __launch_bounds__(kThreads) k_dr_paint(const Prim* __restrict__ sorted, int32_t P, int H, int W, int tiles_x, int tiles_per_frame,
                                                       const uint8_t* __restrict__ background, int64_t background_stride, uint32_t bg_color,
                                                       uint8_t* __restrict__ rgb) {
    __shared__ Prim s_prim[kThreads];
    __shared__ int s_wave[kThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t tile = blockIdx.x;
    const int64_t b = tile / tiles_per_frame;
    const int tl = (int)(tile - b * tiles_per_frame);
    const int ty = tl / tiles_x, tx = tl - ty * tiles_x;
    const int x0 = tx * kTileW, y0 = ty * kTileH;
    const int x = x0 + 4 * (tid % kLanesX), y = y0 + tid / kLanesX;
    const bool live = x < W && y < H;
    const int npx = live ? min(4, W - x) : 0;             // (kDwords: 4 whenever live)
    const int64_t pix = ((int64_t)b * H + y) * (int64_t)W + x;

    float c[12];
    if (live) {
        if (background) {
            const uint8_t* bg = background + b * background_stride + ((int64_t)y * W + x) * 3;
            uint8_t v[12];
            if (kDwords) {
                load12(bg, true, v);
            } else {
#pragma unroll
                for (int i = 0; i < 12; ++i) v[i] = i < 3 * npx ? bg[i] : 0;
            }
#pragma unroll
            for (int i = 0; i < 12; ++i) c[i] = (float)v[i];
        } else {
#pragma unroll
            for (int i = 0; i < 12; ++i) c[i] = (float)((bg_color >> (8 * (i % 3))) & 0xffu);
        }
    }
    // the tile's box of pixel centres
    const float cx0 = (float)x0 + 0.5f, cx1 = (float)(min(x0 + kTileW, W) - 1) + 0.5f;
    const float cy0 = (float)y0 + 0.5f, cy1 = (float)(min(y0 + kTileH, H) - 1) + 0.5f;
    const Prim* fp = sorted + b * (int64_t)P;
    for (int p0 = 0; p0 < P; p0 += kThreads) {
        // stage: keep the primitives that can cover a centre of the tile (coverage > 0 needs d < r + 0.5), in paint order
        Prim pr;
        bool hit = false;
        if (p0 + tid < P) {
            pr = fp[p0 + tid];
            const float pad = pr.r + 0.5f;
            hit = pr.r >= 0.f && fminf(pr.ax, pr.bx) - pad < cx1 && fmaxf(pr.ax, pr.bx) + pad > cx0 && fminf(pr.ay, pr.by) - pad < cy1 &&
                  fmaxf(pr.ay, pr.by) + pad > cy0;
        }
        const unsigned long long m = __ballot(hit);
        if (lane == 0) s_wave[wave] = __popcll(m);
        __syncthreads();
        int base = 0, n = 0;
#pragma unroll
        for (int w = 0; w < kThreads / 64; ++w) {
            const int cw = s_wave[w];
            base += w < wave ? cw : 0;
            n += cw;
        }
        if (hit) s_prim[base + __popcll(m & ((1ull << lane) - 1ull))] = pr;
        __syncthreads();
        if (live) {
            const float py = (float)y + 0.5f;
            for (int k = 0; k < n; ++k) {
                const Prim q = s_prim[k];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float a = coverage(q, (float)(x + i) + 0.5f, py);
                    if (a > 0.f) {
                        const float na = 1.0f - a;
                        c[3 * i] = c[3 * i] * na + q.cr * a;
                        c[3 * i + 1] = c[3 * i + 1] * na + q.cg * a;
                        c[3 * i + 2] = c[3 * i + 2] * na + q.cb * a;
                    }
                }
            }
        }
        __syncthreads();                                   // (the next chunk overwrites the staged primitives)
    }
    if (!live) return;
    uint8_t v[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) v[i] = (uint8_t)rintf(c[i]);
    uint8_t* o = rgb + pix * 3;
    if (kDwords) {
        store12(o, v);
    } else {
#pragma unroll
        for (int i = 0; i < 12; ++i)
            if (i < 3 * npx) o[i] = v[i];
    }
}

// ---- compositor ----------------------------------------------------------------------------------------------------------------------
struct PanelDev {
    const uint8_t* src;
    int64_t src_stride;
    const uint8_t* strip;
    int32_t src_w;
    int32_t crop_x, crop_y, crop_w, crop_h;
    int32_t resize_h, resize_w;
    int32_t cell_h, cell_w;
    int32_t strip_h, x_offset;
    int32_t dx, dy;                       // resized column = cell column + dx, resized row = cell row + dy
    float scale_x, scale_y;               // crop / resize
    uint32_t fill;
    int32_t resample;
};

struct ComposeDev {
    PanelDev p[DPOSER_MAX_PANELS];
    int32_t n;
};

__device__ __forceinline__ void put3(uint8_t* v, uint32_t rgbx) {
    v[0] = (uint8_t)rgbx; v[1] = (uint8_t)(rgbx >> 8); v[2] = (uint8_t)(rgbx >> 16);
}

__device__ __forceinline__ void panel_pixel(const PanelDev& p, int64_t n, int xc, int y, uint8_t* v) {
    if (y >= p.cell_h) {                                   // the strip under the cell
        const uint8_t* s = p.strip + ((int64_t)(y - p.cell_h) * p.cell_w + xc) * 3;
        v[0] = s[0]; v[1] = s[1]; v[2] = s[2];
        return;
    }
    const int col = xc + p.dx, row = y + p.dy;
    if (col < 0 || col >= p.resize_w || row < 0 || row >= p.resize_h) {
        put3(v, p.fill);
        return;
    }
    const uint8_t* S = p.src + n * p.src_stride;
    if (!p.resample) {
        const uint8_t* s = S + ((int64_t)(p.crop_y + row) * p.src_w + (p.crop_x + col)) * 3;
        v[0] = s[0]; v[1] = s[1]; v[2] = s[2];
        return;
    }
    const float u = ((float)col + 0.5f) * p.scale_x - 0.5f, w = ((float)row + 0.5f) * p.scale_y - 0.5f;
    const float fu = floorf(u), fw = floorf(w);
    const float fx = u - fu, fy = w - fw;
    const int i0 = (int)fu, k0 = (int)fw;
    const int xa = min(max(i0, 0), p.crop_w - 1), xb = min(max(i0 + 1, 0), p.crop_w - 1);
    const int ya = min(max(k0, 0), p.crop_h - 1), yb = min(max(k0 + 1, 0), p.crop_h - 1);
    const uint8_t* r0 = S + ((int64_t)(p.crop_y + ya) * p.src_w + p.crop_x) * 3;
    const uint8_t* r1 = S + ((int64_t)(p.crop_y + yb) * p.src_w + p.crop_x) * 3;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const float p00 = (float)r0[xa * 3 + ch], p01 = (float)r0[xb * 3 + ch], p10 = (float)r1[xa * 3 + ch], p11 = (float)r1[xb * 3 + ch];
        const float top = (1.0f - fx) * p00 + fx * p01, bot = (1.0f - fx) * p10 + fx * p11;
        v[ch] = (uint8_t)rintf(fminf(fmaxf((1.0f - fy) * top + fy * bot, 0.f), 255.f));
    }
}

template <bool kDwords>
__global__ void __launch_bounds__(kThreads) k_cp_compose(ComposeDev cd, int H, int W, int groups_x, int64_t n_groups, uint32_t out_fill,
                                                         uint8_t* __restrict__ out) {
    const int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x;        // group of four pixels: (frame, row, column group)
    if (g >= n_groups) return;
    const int64_t row_id = g / groups_x;
    const int x = 4 * (int)(g - row_id * groups_x);
    const int64_t n = row_id / H;
    const int y = (int)(row_id - n * H);
    const int npx = min(4, W - x);
    uint8_t v[12];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        uint8_t* vi = v + 3 * i;
        put3(vi, out_fill);
        if (i >= npx) continue;
        const int xi = x + i;
        int owner = -1;
        for (int k = 0; k < cd.n; ++k)
            if (xi >= cd.p[k].x_offset && xi < cd.p[k].x_offset + cd.p[k].cell_w && y < cd.p[k].cell_h + cd.p[k].strip_h) owner = k;
        if (owner >= 0) panel_pixel(cd.p[owner], n, xi - cd.p[owner].x_offset, y, vi);
    }
    uint8_t* o = out + (row_id * (int64_t)W + x) * 3;
    if (kDwords) {
        store12(o, v);
    } else {
#pragma unroll
        for (int i = 0; i < 12; ++i)
            if (i < 3 * npx) o[i] = v[i];
    }
}

inline uint32_t pack_rgb(const uint8_t* c) { return (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16); }

}  // namespace

extern "C" int64_t dposer_draw_skeletons_scratch_bytes(int64_t batch, int32_t num_joints, int32_t num_bones) {
    if (batch < 0 || num_joints < 0 || num_bones < 0 || (int64_t)num_joints + num_bones > DPOSER_DRAW_MAX_PRIMITIVES) return 0;
    const int64_t P = (int64_t)num_joints + num_bones;
    return round_up((batch > 0 ? batch : 1) * (P > 0 ? P : 1) * (int64_t)sizeof(Prim), 256);
}

extern "C" int dposer_draw_skeletons(const dposer_draw_skeletons_args* a, void* stream) {
    DP_RANGE();
    DP_CHECK_ARG(a != nullptr, "args is NULL");
    DP_CHECK_ARG(a->batch >= 0, "batch must be >= 0");
    DP_CHECK_ARG(a->num_joints >= 0 && a->num_bones >= 0, "num_joints and num_bones must be >= 0");
    DP_CHECK_ARG((int64_t)a->num_joints + a->num_bones <= DPOSER_DRAW_MAX_PRIMITIVES, "too many primitives (num_bones + num_joints) for one call");
    DP_CHECK_ARG(a->height > 0 && a->width > 0, "height and width must be > 0");
    DP_CHECK_ARG(std::isfinite(a->s) && std::isfinite(a->X0) && std::isfinite(a->Y0) && std::isfinite(a->cx) && std::isfinite(a->cy),
                 "the view must be finite");
    DP_CHECK_ARG(a->line_width >= 0.f && a->joint_radius >= 0.f && std::isfinite(a->line_width) && std::isfinite(a->joint_radius),
                 "line_width and joint_radius must be finite and >= 0");
    DP_CHECK_ARG(a->background_stride >= 0, "background_stride must be >= 0");
    if (a->batch == 0) return DPOSER_OK;
    DP_CHECK_ARG(a->rgb && a->scratch, "rgb and scratch are required");
    DP_CHECK_ARG(((uintptr_t)a->scratch & 255) == 0, "scratch must be 256-byte aligned");
    const int32_t J = a->num_joints, K = a->num_bones, P = J + K, H = a->height, W = a->width;
    DP_CHECK_ARG(J == 0 || (a->joints && a->joint_color), "joints and joint_color are required");
    DP_CHECK_ARG(K == 0 || (J > 0 && a->bones && a->bone_color), "bones and bone_color are required");
    const int tiles_x = (int)ceil_div(W, kTileW), tiles_y = (int)ceil_div(H, kTileH);
    const int64_t tiles_per_frame = (int64_t)tiles_x * tiles_y;
    DP_CHECK_ARG(tiles_per_frame <= INT32_MAX && a->batch <= INT32_MAX / tiles_per_frame, "too many image tiles for one call (split the batch)");
    hipStream_t st = (hipStream_t)stream;
    Prim* sorted = (Prim*)a->scratch;
    if (P > 0) {
        const View vw = {a->s, a->X0, a->Y0, a->cx, a->cy, a->y_up, a->z_toward_viewer};
        hipLaunchKernelGGL(k_dr_prepare, dim3((unsigned)a->batch), dim3(kThreads), 0, st, a->joints, J, K, a->visible, a->bones, a->bone_color,
                           a->joint_color, vw, 0.5f * a->line_width, a->joint_radius, sorted);
        DP_CHECK_LAUNCH();
    }
    const bool dwords = W % 4 == 0 && ((uintptr_t)a->rgb & 3) == 0 &&
                        (!a->background || (((uintptr_t)a->background & 3) == 0 && a->background_stride % 4 == 0));
    const uint32_t bgc = pack_rgb(a->background_color);
    const unsigned grid = (unsigned)(a->batch * tiles_per_frame);
    if (dwords)
        hipLaunchKernelGGL(k_dr_paint<true>, dim3(grid), dim3(kThreads), 0, st, (const Prim*)sorted, P, H, W, tiles_x, (int)tiles_per_frame,
                           a->background, a->background_stride, bgc, a->rgb);
    else
        hipLaunchKernelGGL(k_dr_paint<false>, dim3(grid), dim3(kThreads), 0, st, (const Prim*)sorted, P, H, W, tiles_x, (int)tiles_per_frame,
                           a->background, a->background_stride, bgc, a->rgb);
    DP_CHECK_LAUNCH();
    return DPOSER_OK;
}

extern "C" int dposer_compose_panels(const dposer_compose_args* a, void* stream) {
    DP_RANGE();
    DP_CHECK_ARG(a != nullptr, "args is NULL");
    DP_CHECK_ARG(a->num_frames >= 0, "num_frames must be >= 0");
    DP_CHECK_ARG(a->num_panels >= 0 && a->num_panels <= DPOSER_MAX_PANELS, "num_panels must lie in [0, DPOSER_MAX_PANELS]");
    DP_CHECK_ARG(a->num_panels == 0 || a->panels, "panels is NULL");
    DP_CHECK_ARG(a->out_h > 0 && a->out_w > 0, "out_h and out_w must be > 0");
    ComposeDev cd;
    cd.n = a->num_panels;
    for (int k = 0; k < a->num_panels; ++k) {
        const dposer_panel& p = a->panels[k];
        DP_CHECK_ARG(p.src != nullptr, "a panel's src is NULL");
        DP_CHECK_ARG(p.src_stride >= 0, "src_stride must be >= 0");
        DP_CHECK_ARG(p.src_h > 0 && p.src_w > 0, "src_h and src_w must be > 0");
        DP_CHECK_ARG(p.crop_w > 0 && p.crop_h > 0 && p.crop_x >= 0 && p.crop_y >= 0 && (int64_t)p.crop_x + p.crop_w <= p.src_w &&
                         (int64_t)p.crop_y + p.crop_h <= p.src_h,
                     "a panel's crop must be non-empty and lie inside its source");
        DP_CHECK_ARG(p.resize_h > 0 && p.resize_w > 0 && p.cell_h > 0 && p.cell_w > 0, "resize and cell sizes must be > 0");
        DP_CHECK_ARG(p.strip_h >= 0 && (p.strip_h == 0 || p.strip), "strip is NULL");
        DP_CHECK_ARG(p.x_offset >= 0 && (int64_t)p.x_offset + p.cell_w <= a->out_w && (int64_t)p.cell_h + p.strip_h <= a->out_h,
                     "a panel must lie inside the output");
        PanelDev& d = cd.p[k];
        d.src = p.src; d.src_stride = p.src_stride; d.strip = p.strip; d.src_w = p.src_w;
        d.crop_x = p.crop_x; d.crop_y = p.crop_y; d.crop_w = p.crop_w; d.crop_h = p.crop_h;
        d.resize_h = p.resize_h; d.resize_w = p.resize_w; d.cell_h = p.cell_h; d.cell_w = p.cell_w;
        d.strip_h = p.strip_h; d.x_offset = p.x_offset;
        d.dx = p.resize_w > p.cell_w ? (p.resize_w - p.cell_w) / 2 : -((p.cell_w - p.resize_w) / 2);
        d.dy = p.resize_h - p.cell_h;                      // taller: the bottom rows; shorter: bottom-aligned
        d.scale_x = (float)p.crop_w / (float)p.resize_w;
        d.scale_y = (float)p.crop_h / (float)p.resize_h;
        d.fill = pack_rgb(p.fill);
        d.resample = (p.resize_h != p.crop_h || p.resize_w != p.crop_w) ? 1 : 0;
    }
    if (a->num_frames == 0) return DPOSER_OK;
    DP_CHECK_ARG(a->out != nullptr, "out is NULL");
    const int groups_x = (int)ceil_div(a->out_w, 4);
    const int64_t n_groups = a->num_frames * a->out_h * (int64_t)groups_x;
    const int64_t blocks = ceil_div(n_groups, kThreads);
    DP_CHECK_ARG(blocks <= INT32_MAX, "too many output pixels for one call (split the frames)");
    const bool dwords = a->out_w % 4 == 0 && ((uintptr_t)a->out & 3) == 0;
    const uint32_t fill = pack_rgb(a->out_fill);
    hipStream_t st = (hipStream_t)stream;
    if (dwords)
        hipLaunchKernelGGL(k_cp_compose<true>, dim3((unsigned)blocks), dim3(kThreads), 0, st, cd, a->out_h, a->out_w, groups_x, n_groups, fill, a->out);
    else
        hipLaunchKernelGGL(k_cp_compose<false>, dim3((unsigned)blocks), dim3(kThreads), 0, st, cd, a->out_h, a->out_w, groups_x, n_groups, fill, a->out);
    DP_CHECK_LAUNCH();
    return DPOSER_OK;
}
