// dposer_mesh_self_intersections -- the SI metric of run/demo.py:148-161 (lib/utils/metric.py:41-92): which faces of B meshes that share one
// face list intersect another face of their mesh, and how many per mesh.  The pair rule is the header's (include/dposer_hip.h); all fp32.
//
//   k_si_faces       face table in tile order: (v0, v1, v2, original face id), id -1 for a degenerate face or a pad slot.
//   k_si_tile_boxes  one wave per (mesh, tile of 64 faces): the union of the tile's face boxes.
//   k_si_pairs       one wave per (mesh, i-tile): walks the j-tiles j >= i whose box meets the i-tile's box (all of them under
//                    DPOSER_SI_ALLPAIRS=1), stages each in LDS, and tests the lane's i-face against the 64 j-faces: closed-box rejection,
//                    then the exact test.  A hit flags both faces; every writer stores 1, so the races between waves are benign.
//   k_si_count       one block per mesh: flagged faces.
// A tile box is the union of exact per-face min / max, so a face pair whose boxes meet lies in tiles whose boxes meet: culling drops only
// pairs the closed-box test rejects anyway, and the flags are those of the all-pairs walk bit for bit.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <string>

#include "common.h"

namespace {

constexpr int kTile = 64;                 // faces per tile = lanes per wave
constexpr float kBaryEps = 1e-6f;         // interior margin of the one-shared-vertex test

struct SiTuning {
    bool all_pairs = false;               // DPOSER_SI_ALLPAIRS=1: walk every tile pair (no tile culling; A/B and the culling cross-check)
    void load() {
        const char* e = getenv("DPOSER_SI_ALLPAIRS");
        all_pairs = e && e[0] == '1';
    }
};
SiTuning& si_tuning() {
    static SiTuning t = [] { SiTuning x; x.load(); return x; }();
    return t;
}

struct V3 { float x, y, z; };
__device__ __forceinline__ V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ float comp(V3 a, int i) { return i == 0 ? a.x : (i == 1 ? a.y : a.z); }
__device__ __forceinline__ bool same_sign(float a, float b) { return (a > 0.f && b > 0.f) || (a < 0.f && b < 0.f); }   // a * b > 0, no underflow

// segment A -> B against triangle (q0, q1, q2), Moller-Trumbore: crosses it at barycentric (b1, b2) on (q1, q2) strictly inside
__device__ bool si_segment_interior(V3 A, V3 B, V3 q0, V3 q1, V3 q2) {
    const V3 e1 = sub(q1, q0), e2 = sub(q2, q0), d = sub(B, A);
    const V3 pv = cross(d, e2);
    const float det = dot(e1, pv);
    if (det == 0.f) return false;                                  // parallel to the plane
    const float inv = 1.0f / det;
    const V3 tv = sub(A, q0);
    const float b1 = dot(tv, pv) * inv;
    const V3 qv = cross(tv, e1);
    const float b2 = dot(d, qv) * inv;
    const float t = dot(e2, qv) * inv;
    return t >= 0.f && t <= 1.f && b1 > kBaryEps && b2 > kBaryEps && b1 + b2 < 1.0f;
}

// face p (shared vertex at corner k) against face q: the segment between the midpoints of p's two edges at the shared vertex
__device__ bool si_shared_vertex(const V3 (&p)[3], int k, const V3 (&q)[3]) {
    const V3 s = p[k], a = p[k == 2 ? 0 : k + 1], b = p[k == 0 ? 2 : k - 1];
    const V3 A = {0.5f * s.x + 0.5f * a.x, 0.5f * s.y + 0.5f * a.y, 0.5f * s.z + 0.5f * a.z};
    const V3 B = {0.5f * s.x + 0.5f * b.x, 0.5f * s.y + 0.5f * b.y, 0.5f * s.z + 0.5f * b.z};
    return si_segment_interior(A, B, q[0], q[1], q[2]);
}

// Moller, "A fast triangle-triangle intersection test" (1997): coplanar branch
__device__ bool si_edge_edge(float Ax, float Ay, V3 v0, V3 u0, V3 u1, int i0, int i1) {
    const float Bx = comp(u0, i0) - comp(u1, i0), By = comp(u0, i1) - comp(u1, i1);
    const float Cx = comp(v0, i0) - comp(u0, i0), Cy = comp(v0, i1) - comp(u0, i1);
    const float f = Ay * Bx - Ax * By, d = By * Cx - Bx * Cy;
    if ((f > 0.f && d >= 0.f && d <= f) || (f < 0.f && d <= 0.f && d >= f)) {
        const float e = Ax * Cy - Ay * Cx;
        if (f > 0.f) return e >= 0.f && e <= f;
        return e <= 0.f && e >= f;
    }
    return false;
}
__device__ bool si_edge_tri(V3 v0, V3 v1, const V3 (&u)[3], int i0, int i1) {
    const float Ax = comp(v1, i0) - comp(v0, i0), Ay = comp(v1, i1) - comp(v0, i1);
    return si_edge_edge(Ax, Ay, v0, u[0], u[1], i0, i1) || si_edge_edge(Ax, Ay, v0, u[1], u[2], i0, i1) ||
           si_edge_edge(Ax, Ay, v0, u[2], u[0], i0, i1);
}
__device__ bool si_point_in_tri(V3 p, const V3 (&u)[3], int i0, int i1) {
    float d[3];
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        const V3 a0 = u[e], a1 = u[e == 2 ? 0 : e + 1];
        const float a = comp(a1, i1) - comp(a0, i1), b = -(comp(a1, i0) - comp(a0, i0));
        const float c = -a * comp(a0, i0) - b * comp(a0, i1);
        d[e] = a * comp(p, i0) + b * comp(p, i1) + c;
    }
    return same_sign(d[0], d[1]) && same_sign(d[0], d[2]);
}
__device__ bool si_coplanar(V3 n, const V3 (&v)[3], const V3 (&u)[3]) {
    const float ax = fabsf(n.x), ay = fabsf(n.y), az = fabsf(n.z);
    int i0, i1;                                                    // project onto the axis plane of largest area
    if (ax > ay) {
        if (ax > az) { i0 = 1; i1 = 2; } else { i0 = 0; i1 = 1; }
    } else {
        if (az > ay) { i0 = 0; i1 = 1; } else { i0 = 0; i1 = 2; }
    }
    if (si_edge_tri(v[0], v[1], u, i0, i1) || si_edge_tri(v[1], v[2], u, i0, i1) || si_edge_tri(v[2], v[0], u, i0, i1)) return true;
    return si_point_in_tri(v[0], u, i0, i1) || si_point_in_tri(u[0], v, i0, i1);
}

// interval of triangle (projections p, plane distances d of the other triangle's plane) on the planes' line; false: coplanar
__device__ bool si_interval(const float (&p)[3], const float (&d)[3], float& lo, float& hi) {
    int k;                                                         // the vertex alone on its side
    if (same_sign(d[0], d[1])) k = 2;
    else if (same_sign(d[0], d[2])) k = 1;
    else if (same_sign(d[1], d[2]) || d[0] != 0.f) k = 0;
    else if (d[1] != 0.f) k = 1;
    else if (d[2] != 0.f) k = 2;
    else return false;
    const int k1 = k == 0 ? 1 : 0, k2 = k == 2 ? 1 : 2;
    const float t0 = p[k] + (p[k1] - p[k]) * d[k] / (d[k] - d[k1]);
    const float t1 = p[k] + (p[k2] - p[k]) * d[k] / (d[k] - d[k2]);
    lo = fminf(t0, t1);
    hi = fmaxf(t0, t1);
    return true;
}

// Moller's triangle-triangle test; plane distances as n . (x - corner 0) (the difference form: no cancellation against n . corner 0)
__device__ bool si_tri_tri(const V3 (&v)[3], const V3 (&u)[3]) {
    const V3 n1 = cross(sub(v[1], v[0]), sub(v[2], v[0]));
    float du[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) du[i] = dot(n1, sub(u[i], v[0]));
    if (same_sign(du[0], du[1]) && same_sign(du[0], du[2])) return false;
    const V3 n2 = cross(sub(u[1], u[0]), sub(u[2], u[0]));
    float dv[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) dv[i] = dot(n2, sub(v[i], u[0]));
    if (same_sign(dv[0], dv[1]) && same_sign(dv[0], dv[2])) return false;
    const V3 D = cross(n1, n2);
    const float mx = fabsf(D.x), my = fabsf(D.y), mz = fabsf(D.z);
    const int ax = (my > mx) ? ((mz > my) ? 2 : 1) : ((mz > mx) ? 2 : 0);
    const float vp[3] = {comp(v[0], ax), comp(v[1], ax), comp(v[2], ax)};
    const float up[3] = {comp(u[0], ax), comp(u[1], ax), comp(u[2], ax)};
    float a0, a1, b0, b1;
    if (!si_interval(vp, dv, a0, a1)) return si_coplanar(n1, v, u);
    if (!si_interval(up, du, b0, b1)) return si_coplanar(n1, v, u);
    return !(a1 < b0 || b1 < a0);
}

__device__ __forceinline__ bool key_less(int4 a, int4 b) {       // sorted vertex indices, lexicographic
    int a0 = min(a.x, min(a.y, a.z)), a2 = max(a.x, max(a.y, a.z)), a1 = a.x + a.y + a.z - a0 - a2;
    int b0 = min(b.x, min(b.y, b.z)), b2 = max(b.x, max(b.y, b.z)), b1 = b.x + b.y + b.z - b0 - b2;
    return a0 != b0 ? a0 < b0 : (a1 != b1 ? a1 < b1 : a2 < b2);
}

// the pair rule of the header for two non-degenerate faces (indices fi / gi, corners f / g) whose boxes meet
__device__ bool si_pair(int4 fi, const V3 (&f)[3], int4 gi, const V3 (&g)[3]) {
    const int fv[3] = {fi.x, fi.y, fi.z}, gv[3] = {gi.x, gi.y, gi.z};
    int shared = 0, kf = 0, kg = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            if (fv[i] == gv[j]) { ++shared; kf = i; kg = j; }
    if (shared == 3) return true;
    if (shared == 2) return false;
    if (shared == 1) return si_shared_vertex(f, kf, g) || si_shared_vertex(g, kg, f);
    return key_less(fi, gi) ? si_tri_tri(f, g) : si_tri_tri(g, f);
}

__device__ __forceinline__ V3 load_v3(const float* vb, int v) {
    const float* p = vb + (int64_t)v * 3;
    return {p[0], p[1], p[2]};
}

__global__ void __launch_bounds__(256) k_si_faces(const int32_t* __restrict__ faces, const int32_t* __restrict__ order, int32_t F,
                                                  int64_t slots, int4* __restrict__ table) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= slots) return;
    int4 r = {0, 0, 0, -1};
    if (p < F) {
        const int fid = order ? order[p] : (int)p;
        const int a = faces[(int64_t)fid * 3], b = faces[(int64_t)fid * 3 + 1], c = faces[(int64_t)fid * 3 + 2];
        r = {a, b, c, (a == b || b == c || a == c) ? -1 : fid};
    }
    table[p] = r;
}

// box (min, max) of every tile; an empty tile gets (+inf, -inf), which meets nothing
__global__ void __launch_bounds__(256) k_si_tile_boxes(const float* __restrict__ verts, int32_t V, const int4* __restrict__ table, int32_t T,
                                                       int64_t n_boxes, float4* __restrict__ boxes) {
    const int lane = threadIdx.x & 63;
    const int64_t w = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;      // (mesh, tile)
    if (w >= n_boxes) return;                                                      // (whole waves)
    const int64_t b = w / T;
    const int t = (int)(w - b * T);
    const int4 f = table[(int64_t)t * kTile + lane];
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (f.w >= 0) {
        const float* vb = verts + b * V * 3;
        const V3 p[3] = {load_v3(vb, f.x), load_v3(vb, f.y), load_v3(vb, f.z)};
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            lo[0] = fminf(lo[0], p[i].x); lo[1] = fminf(lo[1], p[i].y); lo[2] = fminf(lo[2], p[i].z);
            hi[0] = fmaxf(hi[0], p[i].x); hi[1] = fmaxf(hi[1], p[i].y); hi[2] = fmaxf(hi[2], p[i].z);
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            lo[c] = fminf(lo[c], __shfl_xor(lo[c], d));
            hi[c] = fmaxf(hi[c], __shfl_xor(hi[c], d));
        }
    if (lane == 0) {
        boxes[2 * w] = float4{lo[0], lo[1], lo[2], 0.f};
        boxes[2 * w + 1] = float4{hi[0], hi[1], hi[2], 0.f};
    }
}

__device__ __forceinline__ bool boxes_meet(float4 alo, float4 ahi, float4 blo, float4 bhi) {
    return alo.x <= bhi.x && blo.x <= ahi.x && alo.y <= bhi.y && blo.y <= ahi.y && alo.z <= bhi.z && blo.z <= ahi.z;
}

__global__ void __launch_bounds__(64) k_si_pairs(const float* __restrict__ verts, int32_t V, int32_t F, const int4* __restrict__ table,
                                                 int32_t T, const float4* __restrict__ boxes, int all_pairs, uint8_t* __restrict__ flags) {
    __shared__ int4 s_idx[kTile];
    __shared__ float4 s_lo[kTile], s_hi[kTile];
    __shared__ float4 s_p[kTile][3];
    const int lane = threadIdx.x;
    const int64_t b = blockIdx.x / T;
    const int it = (int)(blockIdx.x - b * T);
    const float* vb = verts + b * V * 3;
    const float4* mb = boxes + 2 * b * T;
    uint8_t* fb = flags + b * F;

    const int4 fi = table[(int64_t)it * kTile + lane];
    const bool valid_i = fi.w >= 0;
    V3 pi[3] = {};
    float4 ilo = {INFINITY, INFINITY, INFINITY, 0.f}, ihi = {-INFINITY, -INFINITY, -INFINITY, 0.f};
    if (valid_i) {
        pi[0] = load_v3(vb, fi.x); pi[1] = load_v3(vb, fi.y); pi[2] = load_v3(vb, fi.z);
        ilo = {fminf(pi[0].x, fminf(pi[1].x, pi[2].x)), fminf(pi[0].y, fminf(pi[1].y, pi[2].y)), fminf(pi[0].z, fminf(pi[1].z, pi[2].z)), 0.f};
        ihi = {fmaxf(pi[0].x, fmaxf(pi[1].x, pi[2].x)), fmaxf(pi[0].y, fmaxf(pi[1].y, pi[2].y)), fmaxf(pi[0].z, fmaxf(pi[1].z, pi[2].z)), 0.f};
    }
    const float4 tlo = mb[2 * it], thi = mb[2 * it + 1];
    bool flag_i = false;

    for (int jt0 = it; jt0 < T; jt0 += kTile) {
        const int jl = jt0 + lane;
        bool meet = false;
        if (jl < T) meet = all_pairs || boxes_meet(tlo, thi, mb[2 * jl], mb[2 * jl + 1]);
        uint64_t cand = __ballot(meet);
        while (cand) {
            const int jt = jt0 + __builtin_ctzll(cand);
            cand &= cand - 1;
            // stage the j-tile: lane k holds face k's indices, box and corners
            const int4 fj = table[(int64_t)jt * kTile + lane];
            V3 pj[3] = {};
            float4 jlo = {INFINITY, INFINITY, INFINITY, 0.f}, jhi = {-INFINITY, -INFINITY, -INFINITY, 0.f};
            if (fj.w >= 0) {
                pj[0] = load_v3(vb, fj.x); pj[1] = load_v3(vb, fj.y); pj[2] = load_v3(vb, fj.z);
                jlo = {fminf(pj[0].x, fminf(pj[1].x, pj[2].x)), fminf(pj[0].y, fminf(pj[1].y, pj[2].y)), fminf(pj[0].z, fminf(pj[1].z, pj[2].z)), 0.f};
                jhi = {fmaxf(pj[0].x, fmaxf(pj[1].x, pj[2].x)), fmaxf(pj[0].y, fmaxf(pj[1].y, pj[2].y)), fmaxf(pj[0].z, fmaxf(pj[1].z, pj[2].z)), 0.f};
            }
            s_idx[lane] = fj;
            s_lo[lane] = jlo;
            s_hi[lane] = jhi;
#pragma unroll
            for (int c = 0; c < 3; ++c) s_p[lane][c] = float4{pj[c].x, pj[c].y, pj[c].z, 0.f};
            __syncthreads();
            uint64_t jflag = 0;                                    // bit k: face k of the j-tile hit some i-face (wave-uniform)
            const uint64_t jvalid = __ballot(fj.w >= 0);
            for (int k = 0; k < kTile; ++k) {
                if (!((jvalid >> k) & 1)) continue;
                bool hit = false;
                const bool need = valid_i && (jt != it || k > lane) && !(flag_i && ((jflag >> k) & 1));
                if (need && boxes_meet(ilo, ihi, s_lo[k], s_hi[k])) {
                    const int4 gk = s_idx[k];
                    V3 g[3];
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const float4 q = s_p[k][c];
                        g[c] = {q.x, q.y, q.z};
                    }
                    hit = si_pair(fi, pi, gk, g);
                }
                flag_i |= hit;
                if (__ballot(hit)) jflag |= 1ull << k;
            }
            if ((jflag >> lane) & 1) fb[fj.w] = 1;
            __syncthreads();                                       // (the next staging overwrites the tile)
        }
    }
    if (flag_i) fb[fi.w] = 1;
}

__global__ void __launch_bounds__(256) k_si_count(const uint8_t* __restrict__ flags, int32_t F, int32_t* __restrict__ counts) {
    __shared__ int s_sum[4];
    const uint8_t* fb = flags + (int64_t)blockIdx.x * F;
    int n = 0;
    for (int i = threadIdx.x; i < F; i += 256) n += fb[i];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) n += __shfl_xor(n, d);
    if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
}

int64_t si_table_bytes(int32_t F) { return round_up(ceil_div(F, kTile) * kTile * (int64_t)sizeof(int4), 256); }

}  // namespace

void meshsi_tuning_reload() { si_tuning().load(); }

extern "C" int64_t dposer_mesh_self_intersections_scratch_bytes(int64_t batch, int32_t num_faces) {
    if (batch < 0 || num_faces <= 0) return 0;
    return si_table_bytes(num_faces) + round_up(batch * ceil_div(num_faces, kTile) * 2 * (int64_t)sizeof(float4), 256);
}

extern "C" int dposer_mesh_self_intersections(const dposer_mesh_si_args* a, void* stream) {
    DP_RANGE();
    DP_CHECK_ARG(a != nullptr, "args is NULL");
    DP_CHECK_ARG(a->batch >= 0, "batch < 0");
    DP_CHECK_ARG(a->num_faces > 0, "num_faces must be > 0");
    DP_CHECK_ARG(a->num_vertices > 0, "num_vertices must be > 0");
    if (a->batch == 0) return DPOSER_OK;
    DP_CHECK_ARG(a->vertices && a->faces && a->flags && a->counts && a->scratch, "vertices, faces, flags, counts and scratch are required");
    DP_CHECK_ARG(((uintptr_t)a->scratch & 255) == 0, "scratch must be 256-byte aligned");
    const int32_t F = a->num_faces, V = a->num_vertices;
    const int64_t B = a->batch, T = ceil_div(F, kTile);
    DP_CHECK_ARG(B * T <= INT32_MAX && B <= INT32_MAX, "batch x tiles exceeds the grid");
    hipStream_t st = (hipStream_t)stream;
    int4* table = (int4*)a->scratch;
    float4* boxes = (float4*)((char*)a->scratch + si_table_bytes(F));
    const int64_t slots = T * kTile;

    DP_CHECK_HIP(hipMemsetAsync(a->flags, 0, B * F, st));
    hipLaunchKernelGGL(k_si_faces, dim3((unsigned)ceil_div(slots, 256)), dim3(256), 0, st, a->faces, a->face_order, F, slots, table);
    DP_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_si_tile_boxes, dim3((unsigned)ceil_div(B * T, 4)), dim3(256), 0, st, a->vertices, V, (const int4*)table, (int32_t)T,
                       B * T, boxes);
    DP_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_si_pairs, dim3((unsigned)(B * T)), dim3(kTile), 0, st, a->vertices, V, F, (const int4*)table, (int32_t)T,
                       (const float4*)boxes, si_tuning().all_pairs ? 1 : 0, a->flags);
    DP_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_si_count, dim3((unsigned)B), dim3(256), 0, st, (const uint8_t*)a->flags, F, a->counts);
    DP_CHECK_LAUNCH();
    return DPOSER_OK;
}
