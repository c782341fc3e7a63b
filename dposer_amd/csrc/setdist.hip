// dposer_pose_set_distances -- every score that reduces over the matrix of distances d(a_i, b_j) between two pose sets under the APD
// distance of lib/utils/metric.py:8-37: the sum (APD), the k nearest references of each row (dNN, the radii of the k-NN manifold scores)
// and the count of references whose radius covers a row (precision / recall / density / coverage).  The rules are the header's
// (include/dposer_hip.h); the matrix itself is never stored.
//
//   k_setdist_reg<J, KMAX>  one lane owns one row a_i, held in 3 J registers; the workgroup (256 rows) streams tiles of 64 references through
//                           LDS.  Every lane reads the same reference, so the LDS reads broadcast (ds_read_b128 of a 16-byte aligned row).
//   k_setdist_gen<KMAX>     any J <= 128: both sets pass through LDS in chunks of 8 joints; a lane keeps one running distance per reference
//                           of a 32-reference tile in registers, so the joints of a pair are still added in index order.
//   k_setdist_merge_rows    the partial k-lists and covered counts of the column splits, merged per row in split order.
//   k_setdist_merge_sum     the per-workgroup fp64 sums, added in index order by one workgroup.
// Grid: (row blocks, column splits).  A split owns a contiguous range of reference tiles and writes its partial results to scratch; nothing is
// accumulated across workgroups with atomics, so the bits of every output depend on (na, nb, J, k, splits) and the data alone.
// Symmetric form (same set, sum only): a row block skips the tiles left of its own 256 columns and counts the tiles right of them twice.
// Per pair and joint: 3 v_sub, v_mul + 2 v_fma, v_sqrt_f32, v_add -- the issue floor of include/dposer_hip.h's cost note.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "common.h"

namespace {

constexpr int kRows = 256;            // rows per workgroup: one lane per row
constexpr int kRegJ = 22;             // the joint count the register path is compiled for (what APD uses)
constexpr int kTileReg = 64;          // references per LDS tile, register path
constexpr int kTileGen = 32;          // references per LDS tile, general path: one running distance per reference and lane
constexpr int kChunk = 8;             // joints per staged chunk, general path
constexpr int kSub = 16;              // references per fp32 partial sum of a lane before it is widened to fp64 (divides both tiles)
constexpr int kMaxSplits = 64;
constexpr int kMaxK = 8;
constexpr int kMaxJoints = 128;
constexpr int kTargetBlocks = 4096;   // workgroups the library's own split count aims for (256 CUs, a few waves of workgroups)
static_assert(kRows % kTileReg == 0 && kRows % kTileGen == 0, "the symmetric form needs tiles that do not straddle a row block's columns");
static_assert(kTileReg % kSub == 0 && kTileGen % kSub == 0, "fp32 partial sums cover whole sub-tiles");

struct SetDistParams {
    const float* a;
    const float* b;
    const float* radii;
    int64_t na;
    int32_t nb, J, k, splits;
    int32_t same_set, symmetric, want_sum, want_knn, want_cov;
    float inv_j;
    float* part_d;        // [splits, na, k]
    int32_t* part_i;      // [splits, na, k]
    int32_t* part_c;      // [splits, na]
    double* part_s;       // [row blocks, splits]
};

// The k best (smallest) distances seen so far, ascending, in registers.  offer() keeps an earlier candidate in front of a later equal one, so
// with candidates offered in index order ties go to the smaller index; a NaN never passes the first test.
template <int KMAX> struct KBest {
    float d[KMAX > 0 ? KMAX : 1];
    int32_t i[KMAX > 0 ? KMAX : 1];
    __device__ __forceinline__ void init() {
#pragma unroll
        for (int p = 0; p < KMAX; ++p) { d[p] = INFINITY; i[p] = -1; }
    }
    __device__ __forceinline__ void offer(float x, int32_t j) {
        if constexpr (KMAX > 0) {
            if (x < d[KMAX - 1]) {
#pragma unroll
                for (int p = KMAX - 1; p > 0; --p) {
                    const bool shift = x < d[p - 1], here = !shift && x < d[p];      // (d[p] is still the old entry here)
                    d[p] = shift ? d[p - 1] : (here ? x : d[p]);
                    i[p] = shift ? i[p - 1] : (here ? j : i[p]);
                }
                if (x < d[0]) { d[0] = x; i[0] = j; }
            }
        }
    }
};

// one joint's share of the distance: differences formed directly, sum of three squares, one v_sqrt_f32 (1 ulp)
__device__ __forceinline__ float joint_dist(float ax, float ay, float az, float bx, float by, float bz) {
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    return __builtin_amdgcn_sqrtf(fmaf(dz, dz, fmaf(dy, dy, dx * dx)));
}

__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d);       // x + partner: the same bits in both lanes of every step
    return x;
}

// The tiles [t_lo, t_hi) of split s, of tiles_total tiles cut into S near-equal ranges; the symmetric form starts at the row block's own columns.
__device__ __forceinline__ void split_range(const SetDistParams& p, int tile, int64_t row0, int& t_lo, int& t_hi) {
    const int64_t tiles = ((int64_t)p.nb + tile - 1) / tile;
    t_lo = (int)(tiles * blockIdx.y / p.splits);
    t_hi = (int)(tiles * (blockIdx.y + 1) / p.splits);
    if (p.symmetric) {
        const int64_t first = row0 / tile;
        if (first > t_lo) t_lo = (int)(first < t_hi ? first : t_hi);
    }
}

// What a lane does with one finished distance: the same in both paths.
template <int KMAX> struct RowState {
    KBest<KMAX> best;
    int32_t covered;
    double sum;
    float part;           // fp32 sum of the current sub-tile
    __device__ __forceinline__ void init() { best.init(); covered = 0; sum = 0.0; part = 0.0f; }
    __device__ __forceinline__ void take(const SetDistParams& p, float d, int32_t col, int64_t row, float radius) {
        part += d;
        if (!(p.same_set && col == row)) {
            best.offer(d, col);
            if (p.want_cov) covered += d <= radius ? 1 : 0;          // (false for a NaN)
        }
    }
    __device__ __forceinline__ void close_sub(double weight) { sum += (double)part * weight; part = 0.0f; }
};

template <int KMAX>
__device__ __forceinline__ void write_partials(const SetDistParams& p, RowState<KMAX>& st, int64_t row, bool valid, double* s_red) {
    const int s = blockIdx.y;
    if (valid) {
        if (p.want_knn) {
            const int64_t base = ((int64_t)s * p.na + row) * p.k;
#pragma unroll
            for (int q = 0; q < KMAX; ++q)
                if (q < p.k) { p.part_d[base + q] = st.best.d[q]; p.part_i[base + q] = st.best.i[q]; }
        }
        if (p.want_cov) p.part_c[(int64_t)s * p.na + row] = st.covered;
    }
    if (p.want_sum) {
        const double w = wave_sum(valid ? st.sum : 0.0);
        if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = w;
        __syncthreads();
        if (threadIdx.x == 0) {
            double t = s_red[0];
#pragma unroll
            for (int v = 1; v < kRows / 64; ++v) t += s_red[v];
            p.part_s[(int64_t)blockIdx.x * p.splits + s] = t;
        }
    }
}

template <int J, int KMAX>
__global__ __launch_bounds__(kRows) void k_setdist_reg(SetDistParams p) {
    constexpr int J3 = 3 * J, LD = (J3 + 3) & ~3;                    // rows of the tile start 16-byte aligned
    __shared__ __attribute__((aligned(16))) float s_b[kTileReg * LD];
    __shared__ float s_r[kTileReg];
    __shared__ double s_red[kRows / 64];
    const int tid = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * kRows, row = row0 + tid;
    const bool valid = row < p.na;
    float a[J3];
    {
        const float* ar = p.a + (valid ? row : p.na - 1) * J3;        // a lane past the last row repeats it; nothing of it is written
#pragma unroll
        for (int e = 0; e < J3; ++e) a[e] = ar[e];
    }
    RowState<KMAX> st;
    st.init();
    int t_lo, t_hi;
    split_range(p, kTileReg, row0, t_lo, t_hi);
    for (int tile = t_lo; tile < t_hi; ++tile) {
        const int64_t c0 = (int64_t)tile * kTileReg;
        const int tn = (int)(p.nb - c0 < kTileReg ? p.nb - c0 : kTileReg);
        const double weight = p.symmetric && c0 >= row0 + kRows ? 2.0 : 1.0;
        __syncthreads();                                             // the previous tile has been read
        const float* src = p.b + c0 * J3;
        for (int idx = tid; idx < tn * J3; idx += kRows) {
            const int r = idx / J3;
            s_b[r * LD + (idx - r * J3)] = src[idx];
        }
        if (p.want_cov && tid < tn) s_r[tid] = p.radii[c0 + tid];
        __syncthreads();
        for (int t0 = 0; t0 < tn; t0 += kSub) {
            const int t1 = t0 + kSub < tn ? t0 + kSub : tn;
            for (int t = t0; t < t1; ++t) {
                const float* r = s_b + t * LD;
                float s = 0.0f;
#pragma unroll
                for (int j = 0; j < J; ++j) s += joint_dist(a[3 * j], a[3 * j + 1], a[3 * j + 2], r[3 * j], r[3 * j + 1], r[3 * j + 2]);
                st.take(p, s * p.inv_j, (int32_t)(c0 + t), row, p.want_cov ? s_r[t] : 0.0f);
            }
            st.close_sub(weight);
        }
    }
    write_partials(p, st, row, valid, s_red);
}

template <int KMAX>
__global__ __launch_bounds__(kRows) void k_setdist_gen(SetDistParams p) {
    constexpr int C3 = 3 * kChunk, LDA = C3 + 1;                      // odd row stride: the lanes' own rows fall on different banks
    __shared__ float s_a[kRows * LDA];
    __shared__ __attribute__((aligned(16))) float s_b[kChunk * kTileGen * 4];      // [joint of the chunk][reference][x, y, z, -]
    __shared__ float s_r[kTileGen];
    __shared__ double s_red[kRows / 64];
    const int tid = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * kRows, row = row0 + tid;
    const bool valid = row < p.na;
    const int J3 = 3 * p.J;
    RowState<KMAX> st;
    st.init();
    int t_lo, t_hi;
    split_range(p, kTileGen, row0, t_lo, t_hi);
    for (int tile = t_lo; tile < t_hi; ++tile) {
        const int64_t c0 = (int64_t)tile * kTileGen;
        const int tn = (int)(p.nb - c0 < kTileGen ? p.nb - c0 : kTileGen);
        const double weight = p.symmetric && c0 >= row0 + kRows ? 2.0 : 1.0;
        float acc[kTileGen];
#pragma unroll
        for (int t = 0; t < kTileGen; ++t) acc[t] = 0.0f;
        for (int j0 = 0; j0 < p.J; j0 += kChunk) {
            const int jn = p.J - j0 < kChunk ? p.J - j0 : kChunk, w3 = 3 * jn;
            __syncthreads();                                         // the previous chunk has been read
            for (int idx = tid; idx < kRows * w3; idx += kRows) {    // joints j0 .. j0 + jn of the block's rows (rows past the last repeat it)
                const int r = idx / w3, e = idx - r * w3;
                const int64_t rr = row0 + r < p.na ? row0 + r : p.na - 1;
                s_a[r * LDA + e] = p.a[rr * J3 + 3 * j0 + e];
            }
            for (int idx = tid; idx < kTileGen * w3; idx += kRows) { // ... and of the tile's references; slots past the last reference hold zeros
                const int r = idx / w3, e = idx - r * w3;
                s_b[((e / 3) * kTileGen + r) * 4 + e % 3] = r < tn ? p.b[(c0 + r) * J3 + 3 * j0 + e] : 0.0f;
            }
            if (j0 == 0 && p.want_cov && tid < tn) s_r[tid] = p.radii[c0 + tid];
            __syncthreads();
            float av[C3];
#pragma unroll
            for (int e = 0; e < C3; ++e) av[e] = e < w3 ? s_a[tid * LDA + e] : 0.0f;
#pragma unroll
            for (int jj = 0; jj < kChunk; ++jj) {
                if (jj >= jn) break;                                 // (wave-uniform)
#pragma unroll
                for (int t = 0; t < kTileGen; ++t) {
                    const f32x4 bq = *reinterpret_cast<const f32x4*>(s_b + (jj * kTileGen + t) * 4);
                    acc[t] += joint_dist(av[3 * jj], av[3 * jj + 1], av[3 * jj + 2], bq[0], bq[1], bq[2]);
                }
            }
        }
#pragma unroll
        for (int t = 0; t < kTileGen; ++t) {
            if (t < tn) st.take(p, acc[t] * p.inv_j, (int32_t)(c0 + t), row, p.want_cov ? s_r[t] : 0.0f);
            if (t % kSub == kSub - 1) st.close_sub(weight);
        }
    }
    write_partials(p, st, row, valid, s_red);
}

__global__ __launch_bounds__(kRows) void k_setdist_merge_rows(SetDistParams p, float* __restrict__ knn_dist, int32_t* __restrict__ knn_idx,
                                                                int32_t* __restrict__ covered) {
    const int64_t row = (int64_t)blockIdx.x * kRows + threadIdx.x;
    if (row >= p.na) return;
    if (p.want_knn) {
        KBest<kMaxK> best;
        best.init();
        for (int s = 0; s < p.splits; ++s) {                          // split order = index order: an equal distance of a later split stays behind
            const int64_t base = ((int64_t)s * p.na + row) * p.k;
            for (int q = 0; q < p.k; ++q) best.offer(p.part_d[base + q], p.part_i[base + q]);
        }
#pragma unroll
        for (int q = 0; q < kMaxK; ++q)
            if (q < p.k) {
                if (knn_dist) knn_dist[row * p.k + q] = best.d[q];
                if (knn_idx) knn_idx[row * p.k + q] = best.i[q];
            }
    }
    if (p.want_cov) {
        int32_t c = 0;
        for (int s = 0; s < p.splits; ++s) c += p.part_c[(int64_t)s * p.na + row];
        covered[row] = c;
    }
}

// n partial sums -> one: thread t adds partials t, t + 256, ... in that order, then the fixed tree of wave_sum and the waves in order.
__global__ __launch_bounds__(kRows) void k_setdist_merge_sum(const double* __restrict__ part, int64_t n, double* __restrict__ out) {
    __shared__ double s_red[kRows / 64];
    double t = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += kRows) t += part[i];
    t = wave_sum(t);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
        double r = s_red[0];
#pragma unroll
        for (int v = 1; v < kRows / 64; ++v) r += s_red[v];
        out[0] = r;
    }
}

struct Plan {
    int rows, tile, splits, reg;
    int64_t tiles, row_blocks;
};

// Pure function of its arguments; false = refused.
bool make_plan(int64_t na, int64_t nb, int32_t J, int32_t k, Plan& pl) {
    if (na < 1 || nb < 1 || nb >= ((int64_t)1 << 31) || J < 1 || J > kMaxJoints || k < 0 || k > kMaxK) return false;
    pl.rows = kRows;
    pl.reg = J == kRegJ ? 1 : 0;
    pl.tile = pl.reg ? kTileReg : kTileGen;
    pl.tiles = ceil_div(nb, pl.tile);
    pl.row_blocks = ceil_div(na, kRows);
    if (pl.row_blocks > INT32_MAX) return false;
    int64_t s = ceil_div(kTargetBlocks, pl.row_blocks);                // (a small set is latency-bound: down to one tile per split)
    if (s > pl.tiles) s = pl.tiles;
    if (s > kMaxSplits) s = kMaxSplits;
    pl.splits = (int)s;
    return true;
}

// splits = 0: the plan's; > 0: that many, up to one per tile and kMaxSplits
int resolve_splits(const Plan& pl, int32_t splits) {
    if (splits <= 0) return pl.splits;
    const int64_t cap = pl.tiles < kMaxSplits ? pl.tiles : kMaxSplits;
    return (int)(splits < cap ? splits : cap);
}

struct ScratchLayout {
    int64_t off_d, off_i, off_c, off_s, bytes;
};

ScratchLayout scratch_layout(const Plan& pl, int64_t na, int32_t k, int splits) {
    ScratchLayout L;
    const int64_t list = round_up((int64_t)splits * na * k * 4, 256);
    L.off_d = 0;
    L.off_i = list;
    L.off_c = 2 * list;
    L.off_s = L.off_c + round_up((int64_t)splits * na * 4, 256);
    L.bytes = L.off_s + round_up(pl.row_blocks * splits * 8, 256);
    return L;
}

template <int KMAX> void launch_pass(const Plan& pl, const SetDistParams& p, dim3 grid, hipStream_t st) {
    if (pl.reg)
        hipLaunchKernelGGL((k_setdist_reg<kRegJ, KMAX>), grid, dim3(kRows), 0, st, p);
    else
        hipLaunchKernelGGL((k_setdist_gen<KMAX>), grid, dim3(kRows), 0, st, p);
}

}  // namespace

extern "C" int dposer_pose_set_distances_plan(int64_t na, int64_t nb, int32_t joints, int32_t k, int32_t plan[4]) {
    DP_CHECK_ARG(plan != nullptr, "plan is NULL");
    Plan pl;
    DP_CHECK_ARG(make_plan(na, nb, joints, k, pl), "need na >= 1, 1 <= nb < 2^31, 1 <= joints <= 128, 0 <= k <= 8");
    plan[0] = pl.rows;
    plan[1] = pl.tile;
    plan[2] = pl.splits;
    plan[3] = pl.reg;
    return DPOSER_OK;
}

extern "C" int64_t dposer_pose_set_distances_scratch_bytes(int64_t na, int64_t nb, int32_t joints, int32_t k, int32_t splits) {
    Plan pl;
    if (!make_plan(na, nb, joints, k, pl) || splits < 0)
        return dposer_set_error(DPOSER_ERR_BAD_ARG, "dposer_pose_set_distances_scratch_bytes: need na >= 1, 1 <= nb < 2^31, 1 <= joints <= 128, "
                                                    "0 <= k <= 8, splits >= 0");
    return scratch_layout(pl, na, k, resolve_splits(pl, splits)).bytes;
}

extern "C" int dposer_pose_set_distances(const dposer_set_dist_args* a, void* stream) {
    DP_RANGE();
    DP_CHECK_ARG(a != nullptr, "args is NULL");
    DP_CHECK_ARG(a->a != nullptr, "a is NULL");
    const bool same = a->same_set != 0;
    if (same) {
        DP_CHECK_ARG(a->b == nullptr || a->b == a->a, "same_set: b must be a (or NULL)");
        DP_CHECK_ARG(a->nb == a->na, "same_set: nb must equal na");
    } else {
        DP_CHECK_ARG(a->b != nullptr, "b is NULL");
    }
    const bool want_knn = a->knn_dist || a->knn_idx, want_cov = a->covered != nullptr, want_sum = a->sum != nullptr;
    DP_CHECK_ARG(want_knn || want_cov || want_sum, "sum, knn_dist, knn_idx and covered are all NULL");
    Plan pl;
    DP_CHECK_ARG(make_plan(a->na, a->nb, a->joints, a->k, pl), "need na >= 1, 1 <= nb < 2^31, 1 <= joints <= 128, 0 <= k <= 8");
    DP_CHECK_ARG(!want_knn || a->k >= 1, "knn_dist / knn_idx need 1 <= k <= 8");
    DP_CHECK_ARG(!want_cov || a->radii != nullptr, "covered needs radii");
    DP_CHECK_ARG(a->splits >= 0, "splits must be >= 0");
    DP_CHECK_ARG(a->scratch != nullptr, "scratch is NULL");
    DP_CHECK_ARG(((uintptr_t)a->scratch & 255) == 0, "scratch must be 256-byte aligned");
    DP_CHECK_ARG((((uintptr_t)a->a | (uintptr_t)a->b | (uintptr_t)a->radii | (uintptr_t)a->knn_dist | (uintptr_t)a->knn_idx | (uintptr_t)a->covered) & 3) == 0,
                 "a, b, radii, knn_dist, knn_idx and covered must be 4-byte aligned");
    DP_CHECK_ARG(((uintptr_t)a->sum & 7) == 0, "sum must be 8-byte aligned");
    const int splits = resolve_splits(pl, a->splits);
    const int k = want_knn ? a->k : 0;
    const ScratchLayout L = scratch_layout(pl, a->na, a->k, splits);
    char* scratch = static_cast<char*>(a->scratch);
    SetDistParams p;
    p.a = a->a;
    p.b = same ? a->a : a->b;
    p.radii = a->radii;
    p.na = a->na;
    p.nb = (int32_t)a->nb;
    p.J = a->joints;
    p.k = k;
    p.splits = splits;
    p.same_set = same ? 1 : 0;
    p.symmetric = same && want_sum && !want_knn && !want_cov ? 1 : 0;
    p.want_sum = want_sum ? 1 : 0;
    p.want_knn = want_knn ? 1 : 0;
    p.want_cov = want_cov ? 1 : 0;
    p.inv_j = 1.0f / (float)a->joints;
    p.part_d = reinterpret_cast<float*>(scratch + L.off_d);
    p.part_i = reinterpret_cast<int32_t*>(scratch + L.off_i);
    p.part_c = reinterpret_cast<int32_t*>(scratch + L.off_c);
    p.part_s = reinterpret_cast<double*>(scratch + L.off_s);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)pl.row_blocks, (unsigned)splits);
    const int kmax = k == 0 ? 0 : (k == 1 ? 1 : (k <= 4 ? 4 : 8));       // the list a lane keeps; the first k entries leave
    switch (kmax) {
        case 0: launch_pass<0>(pl, p, grid, st); break;
        case 1: launch_pass<1>(pl, p, grid, st); break;
        case 4: launch_pass<4>(pl, p, grid, st); break;
        default: launch_pass<8>(pl, p, grid, st); break;
    }
    DP_CHECK_LAUNCH();
    if (want_knn || want_cov) {
        hipLaunchKernelGGL(k_setdist_merge_rows, dim3((unsigned)pl.row_blocks), dim3(kRows), 0, st, p, a->knn_dist, a->knn_idx, a->covered);
        DP_CHECK_LAUNCH();
    }
    if (want_sum) {
        hipLaunchKernelGGL(k_setdist_merge_sum, dim3(1), dim3(kRows), 0, st, (const double*)p.part_s, pl.row_blocks * splits, a->sum);
        DP_CHECK_LAUNCH();
    }
    return DPOSER_OK;
}
