// dposer_rigid_align / dposer_regress_joints / dposer_ehf_eval -- the similarity Procrustes alignment of lib/utils/transforms.py:264-286
// (rigid_transform_3D, rigid_align) and the EHF evaluation of lib/dataset/mocap_dataset.py:61-84 (MocapDataset.eval_EHF) for B pairs /
// images in one call.  The rules are the header's (include/dposer_hip.h).
//
//   k_rigid_align<WAVES>  one group of WAVES waves per pair (WAVES = 1: N <= 64, four pairs per 256-thread workgroup; WAVES = 4: one
//                         workgroup per pair).  Pass 1: every thread sums the moments of its points (i = thread, thread + group, ...) in
//                         fp64, shifted by the pair's first point; a butterfly over the wave and a fixed-order sum over the waves give
//                         every thread the same totals.  The group's first thread solves (one-sided Jacobi SVD in fp64) and leaves the
//                         transform, rounded to fp32, in LDS.  Pass 2: aligned points and distances in fp32, the distance sum in fp64
//                         through the same tree.
//   k_regress_joints      one thread per (mesh, row): the row's CSR entries in order, fp64 accumulators, optional rotation, fp32 out.
//   k_ehf_metrics         one thread per image: the two EHF means from the joint sets and the alignment's mean distance.
// No sum uses an atomic and none depends on the grid: the bits of a pair depend on its own data and N alone.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "common.h"

namespace {

constexpr int kMoments = 16;              // sum a (3), sum b (3), sum |a|^2 (1), sum a b^T (9)
constexpr int kAlignBlock = 256;
constexpr int kSweeps = 12;               // cap on the cyclic one-sided Jacobi sweeps of a 3 x 3: converges quadratically, 3-5 sweeps in practice
constexpr double kOrthoTol2 = 1e-31;      // a column pair with cos^2 of its angle below this (3e-16 on the cosine) is left alone

__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d);       // x + partner: the same bits in both lanes of every step
    return x;
}

// rigid_transform_3D from the shifted moments of n points: T = (c, R row-major, t), fp64 throughout, rounded once to fp32.
// a0 / b0: the shift (the pair's first points).
__device__ void solve_similarity(const double (&m)[kMoments], double n, const double (&a0)[3], const double (&b0)[3], float (&T)[13]) {
    const double inv_n = 1.0 / n;
    double ma[3], mb[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) { ma[i] = m[i] * inv_n; mb[i] = m[3 + i] * inv_n; }
    const double var = m[6] * inv_n - (ma[0] * ma[0] + ma[1] * ma[1] + ma[2] * ma[2]);     // sum over axes of the population variance
    double G[3][3], W[3][3];                                        // G = H W, columns of G become orthogonal: H = U S W^T
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            G[i][j] = m[7 + 3 * i + j] * inv_n - ma[i] * mb[j];
            W[i][j] = i == j ? 1.0 : 0.0;
        }
    for (int sweep = 0; sweep < kSweeps; ++sweep) {
        bool rotated = false;
#pragma unroll
        for (int pq = 0; pq < 3; ++pq) {
            const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
            const double alpha = G[0][p] * G[0][p] + G[1][p] * G[1][p] + G[2][p] * G[2][p];
            const double beta = G[0][q] * G[0][q] + G[1][q] * G[1][q] + G[2][q] * G[2][q];
            const double gamma = G[0][p] * G[0][q] + G[1][p] * G[1][q] + G[2][p] * G[2][q];
            if (gamma * gamma <= kOrthoTol2 * alpha * beta) continue;     // orthogonal to rounding already (a NaN falls through and spreads)
            rotated = true;
            const double zeta = (beta - alpha) / (2.0 * gamma);
            const double tt = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
            const double cs = 1.0 / sqrt(1.0 + tt * tt), sn = cs * tt;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const double gp = G[i][p], gq = G[i][q], wp = W[i][p], wq = W[i][q];
                G[i][p] = cs * gp - sn * gq;
                G[i][q] = sn * gp + cs * gq;
                W[i][p] = cs * wp - sn * wq;
                W[i][q] = sn * wp + cs * wq;
            }
        }
        if (!rotated) break;                                        // (depends on the pair's own numbers alone)
    }
    double s[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) s[j] = sqrt(G[0][j] * G[0][j] + G[1][j] * G[1][j] + G[2][j] * G[2][j]);
    // singular values in descending order (columns of G and W move together)
#pragma unroll
    for (int pq = 0; pq < 3; ++pq) {
        const int p = pq == 1 ? 1 : 0, q = pq == 1 ? 2 : 1;        // (0,1) (1,2) (0,1)
        if (s[p] < s[q]) {
            const double ts = s[p]; s[p] = s[q]; s[q] = ts;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const double tg = G[i][p]; G[i][p] = G[i][q]; G[i][q] = tg;
                const double tw = W[i][p]; W[i][p] = W[i][q]; W[i][q] = tw;
            }
        }
    }
    // U: u1 = g1 / s1; u2 = g2 made orthogonal to u1; u3 = +-(u1 x u2), the sign g3 has.  A vanishing s2 or s3 (collinear / coplanar
    // points) leaves u2 / u3 to the completion, which is what any SVD does there.
    double U[3][3];
    if (s[0] > 0.0) {
#pragma unroll
        for (int i = 0; i < 3; ++i) U[i][0] = G[i][0] / s[0];
    } else {
        U[0][0] = s[0] == 0.0 ? 1.0 : s[0];                         // H = 0 (or NaN, which must spread)
        U[1][0] = 0.0; U[2][0] = 0.0;
    }
    double d = G[0][1] * U[0][0] + G[1][1] * U[1][0] + G[2][1] * U[2][0];
    double u2[3] = {G[0][1] - d * U[0][0], G[1][1] - d * U[1][0], G[2][1] - d * U[2][0]};
    double n2 = sqrt(u2[0] * u2[0] + u2[1] * u2[1] + u2[2] * u2[2]);
    if (n2 <= 1e-14 * s[0] || n2 == 0.0) {                          // rank <= 1: any unit vector orthogonal to u1
        const double ax = fabs(U[0][0]), ay = fabs(U[1][0]), az = fabs(U[2][0]);
        const int k = (ax <= ay && ax <= az) ? 0 : (ay <= az ? 1 : 2);       // the axis u1 leans on least
        const double e[3] = {k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0};
        d = e[0] * U[0][0] + e[1] * U[1][0] + e[2] * U[2][0];
#pragma unroll
        for (int i = 0; i < 3; ++i) u2[i] = e[i] - d * U[i][0];
        n2 = sqrt(u2[0] * u2[0] + u2[1] * u2[1] + u2[2] * u2[2]);
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) U[i][1] = u2[i] / n2;
    double u3[3] = {U[1][0] * U[2][1] - U[2][0] * U[1][1], U[2][0] * U[0][1] - U[0][0] * U[2][1], U[0][0] * U[1][1] - U[1][0] * U[0][1]};
    if (G[0][2] * u3[0] + G[1][2] * u3[1] + G[2][2] * u3[2] < 0.0) { u3[0] = -u3[0]; u3[1] = -u3[1]; u3[2] = -u3[2]; }
#pragma unroll
    for (int i = 0; i < 3; ++i) U[i][2] = u3[i];

    double R[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) R[i][j] = W[i][0] * U[j][0] + W[i][1] * U[j][1] + W[i][2] * U[j][2];
    const double det = R[0][0] * (R[1][1] * R[2][2] - R[1][2] * R[2][1]) - R[0][1] * (R[1][0] * R[2][2] - R[1][2] * R[2][0]) +
                       R[0][2] * (R[1][0] * R[2][1] - R[1][1] * R[2][0]);
    if (det < 0.0) {                                                // reflection: negate the last singular value and the last row of V^T
        s[2] = -s[2];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) R[i][j] = W[i][0] * U[j][0] + W[i][1] * U[j][1] - W[i][2] * U[j][2];
    }
    const double c = (s[0] + s[1] + s[2]) / var;
    // t = mean(b) - c R mean(a), with the shift put back
    double ca[3], t[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) ca[i] = a0[i] + ma[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = (b0[i] + mb[i]) - c * (R[i][0] * ca[0] + R[i][1] * ca[1] + R[i][2] * ca[2]);
    bool finite = isfinite(c) && isfinite(t[0]) && isfinite(t[1]) && isfinite(t[2]);
#pragma unroll
    for (int i = 0; i < 9; ++i) finite = finite && isfinite(R[i / 3][i % 3]);
    if (!finite) {                                                  // zero variance (0 / 0) or a non-finite coordinate: the whole pair
#pragma unroll
        for (int i = 0; i < 13; ++i) T[i] = NAN;
        return;
    }
    T[0] = (float)c;
#pragma unroll
    for (int i = 0; i < 9; ++i) T[1 + i] = (float)R[i / 3][i % 3];
#pragma unroll
    for (int i = 0; i < 3; ++i) T[10 + i] = (float)t[i];
}

template <int WAVES>
__global__ void __launch_bounds__(kAlignBlock) k_rigid_align(const float* __restrict__ src, const float* __restrict__ dst, int64_t B, int32_t N,
                                                             float* __restrict__ transform, float* __restrict__ aligned,
                                                             float* __restrict__ mean_dist) {
    constexpr int kGroup = 64 * WAVES;                              // threads per pair
    constexpr int kPairs = kAlignBlock / kGroup;                    // pairs per workgroup
    __shared__ double s_part[kAlignBlock / 64][kMoments];
    __shared__ float s_T[kPairs][13];
    const int g = threadIdx.x / kGroup, tg = threadIdx.x % kGroup, wave = threadIdx.x >> 6;
    const int64_t pair = (int64_t)blockIdx.x * kPairs + g;
    const bool active = pair < B;                                   // (whole groups; every thread still reaches the barriers)
    const float* a = src + (active ? pair : 0) * N * 3;
    const float* b = dst + (active ? pair : 0) * N * 3;
    const double a0[3] = {(double)a[0], (double)a[1], (double)a[2]}, b0[3] = {(double)b[0], (double)b[1], (double)b[2]};

    double m[kMoments];
#pragma unroll
    for (int k = 0; k < kMoments; ++k) m[k] = 0.0;
    for (int i = tg; i < N; i += kGroup) {
        const float* pa = a + (int64_t)i * 3;
        const float* pb = b + (int64_t)i * 3;
        const double x[3] = {(double)pa[0] - a0[0], (double)pa[1] - a0[1], (double)pa[2] - a0[2]};
        const double y[3] = {(double)pb[0] - b0[0], (double)pb[1] - b0[1], (double)pb[2] - b0[2]};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            m[c] += x[c];
            m[3 + c] += y[c];
        }
        m[6] += x[0] * x[0] + x[1] * x[1] + x[2] * x[2];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) m[7 + 3 * r + c] += x[r] * y[c];
    }
#pragma unroll
    for (int k = 0; k < kMoments; ++k) m[k] = wave_sum(m[k]);
    if (WAVES > 1) {
        if ((threadIdx.x & 63) == 0) {
#pragma unroll
            for (int k = 0; k < kMoments; ++k) s_part[wave][k] = m[k];
        }
        __syncthreads();
        if (tg == 0) {
#pragma unroll
            for (int k = 0; k < kMoments; ++k) {
                double t = s_part[0][k];
                for (int w = 1; w < WAVES; ++w) t += s_part[w][k];
                m[k] = t;
            }
        }
    }
    if (tg == 0) {                                                  // the solve: once per pair
        float T[13];
        solve_similarity(m, (double)N, a0, b0, T);
#pragma unroll
        for (int k = 0; k < 13; ++k) s_T[g][k] = T[k];
        if (active && transform) {
#pragma unroll
            for (int k = 0; k < 13; ++k) transform[pair * 13 + k] = T[k];
        }
    }
    __syncthreads();
    if (!aligned && !mean_dist) return;
    float T[13];
#pragma unroll
    for (int k = 0; k < 13; ++k) T[k] = s_T[g][k];
    double dsum = 0.0;
    for (int i = tg; i < N; i += kGroup) {
        const float* pa = a + (int64_t)i * 3;
        const float* pb = b + (int64_t)i * 3;
        const float x = pa[0], y = pa[1], z = pa[2];
        float o[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) o[r] = fmaf(T[0], fmaf(T[1 + 3 * r + 2], z, fmaf(T[1 + 3 * r + 1], y, T[1 + 3 * r] * x)), T[10 + r]);
        if (active && aligned) {
            float* po = aligned + (pair * N + i) * 3;
            po[0] = o[0]; po[1] = o[1]; po[2] = o[2];
        }
        const float dx = o[0] - pb[0], dy = o[1] - pb[1], dz = o[2] - pb[2];
        dsum += (double)sqrtf(fmaf(dz, dz, fmaf(dy, dy, dx * dx)));
    }
    if (!mean_dist) return;                                         // (uniform: no barrier is skipped by part of a workgroup)
    dsum = wave_sum(dsum);
    if (WAVES > 1) {
        __syncthreads();                                            // (s_part is reused)
        if ((threadIdx.x & 63) == 0) s_part[wave][0] = dsum;
        __syncthreads();
        if (tg == 0) {
            dsum = s_part[0][0];
            for (int w = 1; w < WAVES; ++w) dsum += s_part[w][0];
        }
    }
    if (tg == 0 && active) mean_dist[pair] = (float)(dsum / (double)N);
}

// joints[b, r] = sum_k weight[k] vertices[b, col[k]] over the row's CSR entries in order (fp64), then rot (row-major 3 x 3, may be NULL)
__global__ void __launch_bounds__(256) k_regress_joints(const float* __restrict__ verts, int64_t B, int32_t V, const int32_t* __restrict__ row_ptr,
                                                        const int32_t* __restrict__ col, const float* __restrict__ weight, int32_t R,
                                                        const float* __restrict__ rot, float* __restrict__ joints) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= B * R) return;
    const int64_t b = idx / R;
    const int r = (int)(idx - b * R);
    const float* vb = verts + b * V * 3;
    double acc[3] = {0.0, 0.0, 0.0};
    const int k1 = row_ptr[r + 1];
    for (int k = row_ptr[r]; k < k1; ++k) {
        const double w = (double)weight[k];
        const float* p = vb + (int64_t)col[k] * 3;
        acc[0] += w * (double)p[0];
        acc[1] += w * (double)p[1];
        acc[2] += w * (double)p[2];
    }
    float* out = joints + idx * 3;
    if (rot) {
#pragma unroll
        for (int i = 0; i < 3; ++i)
            out[i] = (float)((double)rot[3 * i] * acc[0] + (double)rot[3 * i + 1] * acc[1] + (double)rot[3 * i + 2] * acc[2]);
    } else {
        out[0] = (float)acc[0]; out[1] = (float)acc[1]; out[2] = (float)acc[2];
    }
}

// pa_mpjpe = 1000 mean_dist;  mpjpe = 1000 mean_j || pred_j - pred_pelvis + gt_pelvis - gt_j ||
__global__ void __launch_bounds__(256) k_ehf_metrics(const float* __restrict__ pred, const float* __restrict__ gt, const float* __restrict__ mean_dist,
                                                     int64_t B, int32_t R, int32_t pelvis, float* __restrict__ pa_mpjpe, float* __restrict__ mpjpe) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const float* p = pred + b * R * 3;
    const float* q = gt + b * R * 3;
    const float pp[3] = {p[pelvis * 3], p[pelvis * 3 + 1], p[pelvis * 3 + 2]}, qp[3] = {q[pelvis * 3], q[pelvis * 3 + 1], q[pelvis * 3 + 2]};
    double sum = 0.0;
    for (int j = 0; j < R; ++j) {
        const float dx = ((p[3 * j] - pp[0]) + qp[0]) - q[3 * j];
        const float dy = ((p[3 * j + 1] - pp[1]) + qp[1]) - q[3 * j + 1];
        const float dz = ((p[3 * j + 2] - pp[2]) + qp[2]) - q[3 * j + 2];
        sum += (double)sqrtf(fmaf(dz, dz, fmaf(dy, dy, dx * dx)));
    }
    pa_mpjpe[b] = 1000.0f * mean_dist[b];
    mpjpe[b] = (float)(1000.0 * (sum / (double)R));
}

int launch_rigid_align(const float* src, const float* dst, int64_t B, int32_t N, float* transform, float* aligned, float* mean_dist,
                       hipStream_t st) {
    if (N <= 64) {
        hipLaunchKernelGGL(k_rigid_align<1>, dim3((unsigned)ceil_div(B, 4)), dim3(kAlignBlock), 0, st, src, dst, B, N, transform, aligned,
                           mean_dist);
    } else {
        hipLaunchKernelGGL(k_rigid_align<4>, dim3((unsigned)B), dim3(kAlignBlock), 0, st, src, dst, B, N, transform, aligned, mean_dist);
    }
    DP_CHECK_LAUNCH();
    return DPOSER_OK;
}

int launch_regress(const float* verts, int64_t B, int32_t V, const int32_t* row_ptr, const int32_t* col, const float* weight, int32_t R,
                   const float* rot, float* joints, hipStream_t st) {
    hipLaunchKernelGGL(k_regress_joints, dim3((unsigned)ceil_div(B * R, 256)), dim3(256), 0, st, verts, B, V, row_ptr, col, weight, R, rot,
                       joints);
    DP_CHECK_LAUNCH();
    return DPOSER_OK;
}

int64_t ehf_joint_bytes(int64_t B, int32_t R) { return round_up(B * R * 3 * (int64_t)sizeof(float), 256); }

}  // namespace

extern "C" int dposer_rigid_align(const dposer_rigid_align_args* a, void* stream) {
    DP_RANGE();
    DP_CHECK_ARG(a != nullptr, "args is NULL");
    DP_CHECK_ARG(a->batch >= 0, "batch < 0");
    DP_CHECK_ARG(a->num_points >= 1, "num_points must be >= 1");
    if (a->batch == 0) return DPOSER_OK;
    DP_CHECK_ARG(a->src && a->dst, "src and dst are required");
    DP_CHECK_ARG(a->batch <= INT32_MAX, "batch exceeds the grid");
    return launch_rigid_align(a->src, a->dst, a->batch, a->num_points, a->transform, a->aligned, a->mean_dist, (hipStream_t)stream);
}

extern "C" int dposer_regress_joints(const dposer_regress_joints_args* a, void* stream) {
    DP_RANGE();
    DP_CHECK_ARG(a != nullptr, "args is NULL");
    DP_CHECK_ARG(a->batch >= 0, "batch < 0");
    DP_CHECK_ARG(a->num_vertices > 0 && a->num_rows > 0, "num_vertices and num_rows must be > 0");
    if (a->batch == 0) return DPOSER_OK;
    DP_CHECK_ARG(a->vertices && a->row_ptr && a->col && a->weight && a->joints, "vertices, row_ptr, col, weight and joints are required");
    DP_CHECK_ARG(ceil_div(a->batch * a->num_rows, 256) <= INT32_MAX, "batch x rows exceeds the grid");
    return launch_regress(a->vertices, a->batch, a->num_vertices, a->row_ptr, a->col, a->weight, a->num_rows, nullptr, a->joints,
                          (hipStream_t)stream);
}

extern "C" int64_t dposer_ehf_eval_scratch_bytes(int64_t batch, int32_t num_rows) {
    if (batch < 0 || num_rows <= 0) return 0;
    return 2 * ehf_joint_bytes(batch, num_rows) + round_up(batch * (int64_t)sizeof(float), 256);
}

extern "C" int dposer_ehf_eval(const dposer_ehf_eval_args* a, void* stream) {
    DP_RANGE();
    DP_CHECK_ARG(a != nullptr, "args is NULL");
    DP_CHECK_ARG(a->batch >= 0, "batch < 0");
    DP_CHECK_ARG(a->num_vertices > 0 && a->num_rows > 0, "num_vertices and num_rows must be > 0");
    DP_CHECK_ARG(a->pelvis_row >= 0 && a->pelvis_row < a->num_rows, "pelvis_row out of range");
    if (a->batch == 0) return DPOSER_OK;
    DP_CHECK_ARG(a->pred_vertices && a->gt_vertices && a->row_ptr && a->col && a->weight && a->pa_mpjpe && a->mpjpe && a->scratch,
                 "pred_vertices, gt_vertices, row_ptr, col, weight, pa_mpjpe, mpjpe and scratch are required");
    DP_CHECK_ARG(((uintptr_t)a->scratch & 255) == 0, "scratch must be 256-byte aligned");
    DP_CHECK_ARG(a->batch <= INT32_MAX && ceil_div(a->batch * a->num_rows, 256) <= INT32_MAX, "batch exceeds the grid");
    const int64_t B = a->batch;
    const int32_t R = a->num_rows;
    hipStream_t st = (hipStream_t)stream;
    char* sc = (char*)a->scratch;
    float* jp = a->pred_joints ? a->pred_joints : (float*)sc;
    float* jg = a->gt_joints ? a->gt_joints : (float*)(sc + ehf_joint_bytes(B, R));
    float* md = (float*)(sc + 2 * ehf_joint_bytes(B, R));
    DP_TRY(launch_regress(a->pred_vertices, B, a->num_vertices, a->row_ptr, a->col, a->weight, R, nullptr, jp, st));
    DP_TRY(launch_regress(a->gt_vertices, B, a->num_vertices, a->row_ptr, a->col, a->weight, R, a->gt_rotation, jg, st));
    DP_TRY(launch_rigid_align(jp, jg, B, R, nullptr, a->aligned_joints, md, st));
    hipLaunchKernelGGL(k_ehf_metrics, dim3((unsigned)ceil_div(B, 256)), dim3(256), 0, st, (const float*)jp, (const float*)jg, (const float*)md,
                       B, R, a->pelvis_row, a->pa_mpjpe, a->mpjpe);
    DP_CHECK_LAUNCH();
    return DPOSER_OK;
}
