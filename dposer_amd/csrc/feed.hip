// dposer_batch_gather -- the device-resident shuffled data feed of the training loop (run/train.py:70-93 builds a shuffling DataLoader over
// a dataset whose __getitem__ returns one pose; here the dataset lives in HBM and a mini-batch is one launch).  Row r of the output is dataset
// row pi(seed, epoch, base + r); pi is a keyed bijection of [0, N) evaluated in the kernel, per row: no permutation array, no sort, no per-epoch
// work, and any (epoch, position) can be asked for at any time -- a resumed run, or another rank, lands on the same rows without state.
// The rule (a balanced Feistel network on Philox4x32-10, cycle-walked into [0, N)) is stated in include/dposer_hip.h and mirrored in numpy by
// tests/feed_ref.py.
//
// Shape of the kernel: HBM-latency-bound (random rows of 252 / 504 bytes), so what counts is loads in flight.  One wave owns kRowsPerWave
// consecutive output rows: lane j evaluates the permutation of row j (once per row -- the other lanes repeat one of the eight), the row
// indices travel by cross-lane reads, and for each 64-dword chunk of the rows the wave issues all its loads before the first store.  Rows are
// only 4-byte aligned (D = 63, 126), so lanes move dwords: 64 lanes x 4 B = one 256-byte request per row and chunk.
#include "common.h"
#include "rng.h"

namespace {

constexpr int kRowsPerWave = 8;
constexpr int kWavesPerBlock = 4;
constexpr int kFeistelRounds = 4;

// pi(seed, epoch, pos): include/dposer_hip.h "Permutation rule".  half_bits = k / 2 <= 31, N <= 2^62.
__device__ __forceinline__ int64_t feed_permute(int64_t pos, int64_t N, int half_bits, uint32_t epoch, uint64_t seed) {
    const uint32_t mask = (uint32_t)((1ull << half_bits) - 1ull);
    uint64_t x = (uint64_t)pos;
    do {                                    // cycle walk: the domain 2^k is < 4 N, so under 4 evaluations are expected
        uint32_t L = (uint32_t)(x >> half_bits), R = (uint32_t)x & mask;
#pragma unroll
        for (int r = 0; r < kFeistelRounds; ++r) {
            const uint32_t F = philox_at((uint64_t)R | ((uint64_t)epoch << 32), STREAM_FEED, (uint32_t)r, seed).v[0] & mask;
            const uint32_t t = L ^ F;
            L = R;
            R = t;
        }
        x = ((uint64_t)L << half_bits) | (uint64_t)R;
    } while (x >= (uint64_t)N);
    return (int64_t)x;
}

// rows idx[0 .. nrows) of src [*, D] -> dst [nrows, D]; idx lives in lanes 0 .. kRowsPerWave-1 (lanes past nrows-1 hold a valid row too).
// Every lane of the wave is active here.  FULL (nrows == kRowsPerWave, every wave but the last): the stores of a chunk sit in ONE predicated
// block.  Given a block each (a test of j < nrows in front of every store), hipcc puts an s_waitcnt vmcnt(0) in front of every store -- for
// the loads, but stores count in vmcnt too, so each store would wait for the one before it.
template <bool FULL>
__device__ __forceinline__ void copy_rows(const float* __restrict__ src, int32_t D, float* __restrict__ dst, int64_t idx, int nrows, int lane) {
    const float* s[kRowsPerWave];
#pragma unroll
    for (int j = 0; j < kRowsPerWave; ++j) s[j] = src + __shfl(idx, j) * (int64_t)D;         // 64-bit row offset: N * D may pass 2^31
    for (int64_t c = lane; c - lane < D; c += 64) {                                          // wave-uniform trip count
        if (c < D) {
            float v[kRowsPerWave];
#pragma unroll
            for (int j = 0; j < kRowsPerWave; ++j) v[j] = s[j][c];                            // all loads of the chunk in flight ...
#pragma unroll
            for (int j = 0; j < kRowsPerWave; ++j)
                if (FULL || j < nrows) dst[(int64_t)j * D + c] = v[j];                        // ... before the first store
        }
    }
}

__global__ __launch_bounds__(64 * kWavesPerBlock) void k_batch_gather(const float* __restrict__ data, int32_t D, const float* __restrict__ aux,
                                                                       int32_t D_aux, int64_t N, int64_t base, int64_t B, int half_bits,
                                                                       uint32_t epoch, uint64_t seed, float* __restrict__ out,
                                                                       float* __restrict__ aux_out, int64_t* __restrict__ indices) {
    const int lane = threadIdx.x & 63;
    const int64_t r0 = ((int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6)) * kRowsPerWave;
    if (r0 >= B) return;                                                                      // wave-uniform
    const int nrows = (int)(B - r0 < kRowsPerWave ? B - r0 : kRowsPerWave);
    int j = lane & (kRowsPerWave - 1);
    if (j >= nrows) j = nrows - 1;                                                            // a short last wave repeats its last row
    const int64_t idx = feed_permute(base + r0 + j, N, half_bits, epoch, seed);
    if (indices && lane < nrows) indices[r0 + lane] = idx;
    if (nrows == kRowsPerWave) {
        if (out) copy_rows<true>(data, D, out + r0 * D, idx, nrows, lane);
        if (aux_out) copy_rows<true>(aux, D_aux, aux_out + r0 * D_aux, idx, nrows, lane);
    } else {
        if (out) copy_rows<false>(data, D, out + r0 * D, idx, nrows, lane);
        if (aux_out) copy_rows<false>(aux, D_aux, aux_out + r0 * D_aux, idx, nrows, lane);
    }
}

}  // namespace

extern "C" int dposer_batch_gather(const dposer_batch_gather_args* a, void* stream) {
    DP_RANGE();
    DP_CHECK_ARG(a != nullptr, "args is NULL");
    DP_CHECK_ARG(a->N >= 1 && a->N <= ((int64_t)1 << 62), "N must be in [1, 2^62]");
    DP_CHECK_ARG(a->B >= 0, "B < 0");
    DP_CHECK_ARG(a->base >= 0 && a->base <= a->N && a->B <= a->N - a->base, "base + B must lie inside [0, N]");
    DP_CHECK_ARG(a->out || a->aux_out || a->indices, "out, aux_out and indices are all NULL");
    if (a->out) {
        DP_CHECK_ARG(a->data != nullptr, "out needs data");
        DP_CHECK_ARG(a->D >= 1, "D must be >= 1");
        DP_CHECK_ARG((((uintptr_t)a->data | (uintptr_t)a->out) & 3) == 0, "data and out must be 4-byte aligned");
    }
    if (a->aux_out) {
        DP_CHECK_ARG(a->aux != nullptr, "aux_out needs aux");
        DP_CHECK_ARG(a->D_aux >= 1, "D_aux must be >= 1");
        DP_CHECK_ARG(a->N_aux >= a->N, "aux must have at least N rows");
        DP_CHECK_ARG((((uintptr_t)a->aux | (uintptr_t)a->aux_out) & 3) == 0, "aux and aux_out must be 4-byte aligned");
    }
    DP_CHECK_ARG(((uintptr_t)a->indices & 7) == 0, "indices must be 8-byte aligned");
    if (a->B == 0) return DPOSER_OK;
    const int64_t blocks = ceil_div(a->B, (int64_t)kRowsPerWave * kWavesPerBlock);
    DP_CHECK_ARG(blocks <= INT32_MAX, "B exceeds the grid");
    int bits = 0;                                                                             // ceil(log2 N)
    while (bits < 62 && ((int64_t)1 << bits) < a->N) ++bits;
    const int half_bits = bits <= 2 ? 1 : (bits + 1) / 2;                                     // k = max(2, 2 ceil(bits / 2)) = 2 half_bits
    hipLaunchKernelGGL(k_batch_gather, dim3((unsigned)blocks), dim3(64 * kWavesPerBlock), 0, (hipStream_t)stream, a->data, a->D, a->aux, a->D_aux,
                       a->N, a->base, a->B, half_bits, a->epoch, a->seed, a->out, a->aux_out, a->indices);
    DP_CHECK_LAUNCH();
    return DPOSER_OK;
}
