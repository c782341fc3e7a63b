// Elementwise, layout and optimizer kernels of the DPoser score path (gfx950).
// These are HBM-bound: one thread handles a "quad" (4 consecutive channels = 8 or 16 contiguous
// bytes of the fragment-tiled layout), grids are sized to the data, no LDS unless transposing.
//
// Scalar SDE arithmetic mirrors the op order of the reference's fp32 torch expressions
// (lib/algorithms/advanced/sde_lib.py) and is compiled with FMA contraction off so that integer
// indices derived from floats (sigmas[(t*999).long()], model.py:159) agree bit-for-bit.
#include "kernels_api.h"
#include "sde_dev.h"
#include "rng.h"

#pragma clang fp contract(off)

// ------------------------------------------------------------------------------------------------
// SDE scalars (sde_lib.py:122-231)
// ------------------------------------------------------------------------------------------------

template <typename T> __device__ __forceinline__ void store_quad_ft(void* base, int64_t s, int c, int K, f32x4 v) {
    Quad<T>::store(reinterpret_cast<T*>(base) + FT<T>::index(s, c, K), v);
}

// time embedding value for channel e of E (model.py:37-51 positional / :19-21 fourier)
// FAST (bf16 storage): hardware v_sin_f32 / v_cos_f32 on the argument in revolutions.  |arg| <= 999 rad = 159 revolutions,
// inside the instruction's +-256 domain; the fp32 product arg * (1/2pi) is off by <= 1e-5 revolutions (6e-5 rad), two orders
// below the bf16 rounding of the stored embedding.  The fp32 parity mode keeps libm sinf / cosf.
template <bool FAST = false>
__device__ __forceinline__ float temb_from_freq(float label, bool sin_half, float f, int fourier) {
    float arg;
    if (fourier) arg = ((logf(label) * f) * 2.0f) * 3.14159274101257324f;
    else arg = label * f;
    if (FAST && !fourier) {
        const float rev = arg * 0.15915494309189535f;
        return sin_half ? __builtin_amdgcn_sinf(rev) : __builtin_amdgcn_cosf(rev);
    }
    return sin_half ? sinf(arg) : cosf(arg);
}
template <bool FAST = false>
__device__ __forceinline__ float temb_value(float label, int e, int E, const float* freq, int fourier) {
    const int half = E >> 1;
    return temb_from_freq<FAST>(label, e < half, freq[e < half ? e : e - half], fourier);
}

// ------------------------------------------------------------------------------------------------
// weight packing
// ------------------------------------------------------------------------------------------------
// The jobs of a multi-job launch sit at the front of the kernel-argument segment; a wave-uniform index into that segment is a scalar
// load with a dynamic offset.  (Indexing the by-value argument struct itself makes hipcc copy it to scratch, and the select chain the
// first version used instead -- `if (i == blockIdx.y) j = jobs.job[i]` over all 40-48 entries -- cost every block ~2 KB of scalar
// loads: k_reduce_grads took 20 us at ANY batch size for ~13000 mostly idle blocks.)
template <typename Job> __device__ __forceinline__ Job kernarg_job(int index) {
    static_assert(sizeof(Job) % 4 == 0, "jobs are copied as dwords");
    typedef const uint32_t __attribute__((address_space(4))) * ConstWords;                      // constant address space: s_load
    ConstWords w = (ConstWords)__builtin_amdgcn_kernarg_segment_ptr() + (size_t)index * (sizeof(Job) / 4);   // (argument 0 starts the segment)
    union { Job j; uint32_t u[sizeof(Job) / 4]; } c;
#pragma unroll
    for (unsigned i = 0; i < sizeof(Job) / 4; ++i) c.u[i] = w[i];
    return c.j;
}

template <typename T> __device__ __forceinline__ void pack_chunk(const PackJob& j, const float* flat, unsigned char* packed, int64_t chunk) {
    constexpr int EPL = FT<T>::EPL, KBS = FT<T>::KBS;
    const int kblocks = j.kpad / KBS;
    const int lane = (int)(chunk & 63);
    const int64_t blk = chunk >> 6;
    const int kb = (int)(blk % kblocks);
    const int64_t rb = blk / kblocks;
    const int r = (int)(rb * 32 + (lane & 31));
    const int k0 = kb * KBS + (lane >> 5) * EPL;
    const float* src = flat + j.src_off;
    T vals[EPL];
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
        const int k = k0 + e;
        float v = 0.f;
        if (r < j.rows_valid && k < j.cols_valid) v = j.trans ? src[(int64_t)k * j.ld + r] : src[(int64_t)r * j.ld + k];
        if (sizeof(T) == 2 && j.split == 2) v = v - (float)(__bf16)v;          // low part of the two-term bf16 split
        vals[e] = from_f32<T>(v);
    }
    T* dst = reinterpret_cast<T*>(packed + j.dst_off) + FT<T>::index(r, j.koff + k0, j.ktot);
    *reinterpret_cast<u32x4*>(dst) = *reinterpret_cast<u32x4*>(vals);
}
__global__ void __launch_bounds__(256) k_pack(PackJobs jobs, const float* flat, unsigned char* packed) {
    (void)jobs;
    const PackJob j = kernarg_job<PackJob>((int)blockIdx.y);
    const int epl = j.f32 ? 4 : 8;
    const int64_t nchunks = (int64_t)j.rows_pad * j.kpad / epl;
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < nchunks; c += (int64_t)gridDim.x * blockDim.x) {
        if (j.f32) pack_chunk<float>(j, flat, packed, c);
        else pack_chunk<__bf16>(j, flat, packed, c);
    }
}
hipError_t launch_pack(const PackJobs& jobs, const float* flat, void* packed, hipStream_t st) {
    if (jobs.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_pack, dim3(256, jobs.n), dim3(256), 0, st, jobs, flat, reinterpret_cast<unsigned char*>(packed));
    return hipGetLastError();
}

__global__ void k_bias_cat(BiasCatJobs j, const float* flat, float* dst) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= j.n * j.H) return;
    const int l = i / j.H, c = i % j.H;
    int64_t a = j.a_off[0], b = j.b_off[0];
#pragma unroll
    for (int k = 1; k < 8; ++k) { a = (l == k) ? j.a_off[k] : a; b = (l == k) ? j.b_off[k] : b; }
    dst[i] = flat[a + c] + flat[b + c];
}
hipError_t launch_bias_cat(const BiasCatJobs& j, const float* flat, float* dst, hipStream_t st) {
    const int n = j.n * j.H;
    hipLaunchKernelGGL(k_bias_cat, dim3((n + 255) / 256), dim3(256), 0, st, j, flat, dst);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// input preparation
// ------------------------------------------------------------------------------------------------
template <typename T> __global__ void __launch_bounds__(256) k_prep_infer(PrepArgs a) {
    const int qx = a.Dpad >> 2, qe = a.emb ? (a.E >> 2) : 0;
    const int64_t nx = a.Bpad * qx;
    const int64_t total = nx + a.Bpad * qe;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        // x part: quad index fastest (consecutive lanes read consecutive floats of one row-major pose);
        // embedding part: sample index fastest (consecutive lanes write consecutive 16-B chunks of an FT block)
        const int64_t s = i < nx ? i / qx : (i - nx) % a.Bpad;
        const int q = i < nx ? (int)(i % qx) : qx + (int)((i - nx) / a.Bpad);
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (q < qx) {
            const int c = q * 4;
            if (s < a.B) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (c + r < a.D) v[r] = a.x[s * a.D + c + r];
            }
            store_quad_ft<T>(a.xin, s, c, a.Dpad, v);
        } else {
            const int e = (q - qx) * 4;
            const float label = s < a.B ? a.labels[s] : (a.fourier ? 1.0f : 0.0f);
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = temb_value<sizeof(T) == 2>(label, e + r, a.E, a.freq, a.fourier);
            store_quad_ft<T>(a.emb, s, e, a.E, v);
        }
    }
}
static inline int grid_for(int64_t n, int per_block = 256, int cap = 8192) {
    int64_t g = (n + per_block - 1) / per_block;
    return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}
hipError_t launch_prep_infer(const PrepArgs& a, hipStream_t st) {
    const int64_t total = a.Bpad * ((a.Dpad >> 2) + (a.emb ? (a.E >> 2) : 0));
    if (a.f32) hipLaunchKernelGGL(k_prep_infer<float>, dim3(grid_for(total)), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_prep_infer<__bf16>, dim3(grid_for(total)), dim3(256), 0, st, a);
    return hipGetLastError();
}

struct PrepTrainDev {
    PrepTrainArgs a;
    SdeDev sde;
    float t_scale;   // (T - eps) as fp32
};
constexpr int PREP_EQ = 8;   // embedding quads per thread: the Philox draw of t is shared by 32 embedding values
template <typename T, bool FOURIER> __global__ void __launch_bounds__(256) k_prep_train(PrepTrainDev d) {
    const PrepTrainArgs& a = d.a;
    const int qx = a.Dpad >> 2, qe = a.E >> 2;
    const int ge = (qe + PREP_EQ - 1) / PREP_EQ;      // embedding work items per sample
    const int QD = (a.D + 3) >> 2;
    const int64_t nx = a.Bpad * qx;
    const int64_t total = nx + a.Bpad * ge;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        // x part: quad index fastest (consecutive lanes read consecutive floats of one row-major pose);
        // embedding part: sample index fastest (consecutive lanes write consecutive 16-B chunks of an FT block)
        const int64_t s = i < nx ? i / qx : (i - nx) % a.Bpad;
        float t = a.eps;
        if (s < a.B) {
            if (a.t_in) t = a.t_in[s];
            else {                                          // losses.py:110  t = rand(B)*(T-eps)+eps
                Philox4 r = philox_at((uint64_t)s, STREAM_TRAIN_T, a.step, a.seed);
                t = u01(r.v[0]) * d.t_scale + a.eps;
            }
        }
        if (i < nx) {
            const int q = (int)(i % qx);
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            const int c = q * 4;
            f32x4 z = {0.f, 0.f, 0.f, 0.f};
            if (s < a.B && c < a.D) {
                if (a.z_in) {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (c + r < a.D) z[r] = a.z_in[s * a.D + c + r];
                } else {                                    // losses.py:111  z = randn_like(batch)
                    float n4[4];
                    normals4((uint64_t)s * QD + q, STREAM_TRAIN_Z, a.step, a.seed, n4);
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (c + r < a.D) z[r] = n4[r];
                }
                const SdeAt at = sde_at(d.sde, t);
                const float mc = at.mc, sd = at.sd;
#pragma unroll
                for (int r = 0; r < 4; ++r)                 // losses.py:112-113  x_t = mean + std*z
                    if (c + r < a.D) v[r] = mc * a.x0[s * a.D + c + r] + sd * z[r];
            }
            store_quad_ft<T>(a.xin, s, c, a.Dpad, v);
            *reinterpret_cast<f32x4*>(a.z_out + s * a.Dpad + c) = z;
            if (q == 0) a.t_out[s] = t;
        } else {
            const int g0 = (int)((i - nx) / a.Bpad) * PREP_EQ;
            const float label = d.sde.kind == SDE_VE ? sde_ve_sigma(d.sde.smin, d.sde.ratio, t) : t * 999.0f;     // utils.py:152 / :173 (training: continuous only)
            // all 32 frequencies first: behind a store to `emb` hipcc cannot hoist the next load of `freq` (the two may alias), and the
            // thread walked 32 dependent load -> sin -> store round trips -- 17 us of the kernel at ANY batch size
            const int half = a.E >> 1;
            f32x4 fr[PREP_EQ];
#pragma unroll
            for (int k = 0; k < PREP_EQ; ++k) {
                const int e = (g0 + k) * 4;
                fr[k] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (e < a.E) fr[k] = *reinterpret_cast<const f32x4*>(a.freq + (e < half ? e : e - half));      // (E / 2 is a multiple of 4)
            }
#pragma unroll
            for (int k = 0; k < PREP_EQ; ++k) {
                const int e = (g0 + k) * 4;
                if (e < a.E) {
                    f32x4 v;
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = temb_from_freq<sizeof(T) == 2>(label, e < half, fr[k][r], FOURIER);      // (a template flag: see launch_prep_train)
                    store_quad_ft<T>(a.emb, s, e, a.E, v);
                }
            }
        }
    }
}
hipError_t launch_prep_train(const PrepTrainArgs& a, hipStream_t st) {
    // The embedding kind is a TEMPLATE flag: as a runtime branch the Fourier form kept 64 inlined libm sinf / cosf (Payne-Hanek slow paths
    // included) between the 32 hardware sin / cos the positional waves actually execute -- 10,343 instructions, the executed ones scattered
    // over 70 KB of code, one instruction-cache miss per unrolled element: the waves sat parked for ~10 of the kernel's 17 us at any
    // batch size (tools/small_step_pmc.sh).  The Fourier instantiation (GaussianFourierProjection, model.py:19-21,152-155) pays that.
    PrepTrainDev d;
    d.a = a;
    d.sde = make_sde_dev(a.sde);
    d.t_scale = (float)((double)a.sde.T - (double)a.eps);
    const int64_t total = a.Bpad * ((a.Dpad >> 2) + ((a.E >> 2) + PREP_EQ - 1) / PREP_EQ);
    if (a.fourier) {
        if (a.f32) hipLaunchKernelGGL((k_prep_train<float, true>), dim3(grid_for(total)), dim3(256), 0, st, d);
        else hipLaunchKernelGGL((k_prep_train<__bf16, true>), dim3(grid_for(total)), dim3(256), 0, st, d);
    } else {
        if (a.f32) hipLaunchKernelGGL((k_prep_train<float, false>), dim3(grid_for(total)), dim3(256), 0, st, d);
        else hipLaunchKernelGGL((k_prep_train<__bf16, false>), dim3(grid_for(total)), dim3(256), 0, st, d);
    }
    return hipGetLastError();
}

__global__ void __launch_bounds__(256) k_time_embed(const float* labels, float label0, int64_t n, int64_t npad, const float* freq, int E, int fourier, float* emb) {
    const int qe = E >> 2;
    const int64_t total = npad * qe;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s = i % npad;
        const int e = (int)(i / npad) * 4;
        const float label = s < n ? (labels ? labels[s] : label0) : (fourier ? 1.0f : 0.0f);
        f32x4 v;
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = temb_value(label, e + r, E, freq, fourier);
        store_quad_ft<float>(emb, s, e, E, v);
    }
}
__global__ void __launch_bounds__(256) k_ve_labels(float* t_inout, int n, float smin, float ratio) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) t_inout[i] = sde_ve_sigma(smin, ratio, t_inout[i]);
}
hipError_t launch_ve_labels(float* t_inout, int n, float smin, float ratio, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_ve_labels, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, t_inout, n, smin, ratio);
    return hipGetLastError();
}
hipError_t launch_time_embed(const float* labels, float label0, int64_t n, int64_t npad, const float* freq, int E, int fourier, float* emb, hipStream_t st) {
    hipLaunchKernelGGL(k_time_embed, dim3(grid_for(npad * (E >> 2))), dim3(256), 0, st, labels, label0, n, npad, freq, E, fourier, emb);
    return hipGetLastError();
}


__global__ void __launch_bounds__(256) k_out_model(OutModelArgs a) {
    const int64_t total = a.B * a.D;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s = i / a.D;
        const int c = (int)(i % a.D);
        float v = a.res[s * a.Cp + c];
        if (a.scale_by_sigma) v = v / used_sigma(a.sigmas, a.num_scales, a.labels[s], a.fourier);   // model.py:192-194
        a.out[i] = v;
    }
}
hipError_t launch_out_model(const OutModelArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(k_out_model, dim3(grid_for(a.B * a.D)), dim3(256), 0, st, a);
    return hipGetLastError();
}

// a kernel's arguments together with the SDE's per-launch constants
template <typename A> struct WithSde {
    A a;
    SdeDev sde;
};
// launches one of the kernels that walk the Bpad x (Dpad / 4) quads of the FT-tiled state: fp32 / bf16 storage by a.f32
template <typename A> static hipError_t launch_quads(void (*k32)(WithSde<A>), void (*k16)(WithSde<A>), const A& a, const SdeDev& sde, hipStream_t st) {
    const WithSde<A> d = {a, sde};
    hipLaunchKernelGGL(a.f32 ? k32 : k16, dim3(grid_for(a.Bpad * (a.Dpad >> 2))), dim3(256), 0, st, d);
    return hipGetLastError();
}
// the divisor of the model output at a launch's shared label (model.py:189-194)
template <typename A> __device__ __forceinline__ float launch_usig(const A& a, float label) {
    return a.scale_by_sigma ? used_sigma(a.sigmas, a.num_scales, label, a.scale_by_sigma == 2) : 1.0f;
}
// The per-element chain behind a network evaluation, in the operation order every call site had (this file is built with contraction off):
// the score from post_dense's output: res / used_sigmas (model.py:194), then -model / std, VE: the model itself (utils.py:155,160,162 / :180)
__device__ __forceinline__ float score_of_res(const SdeDev& sde, float res, float usig, float sd_score) { return sde_score(sde, res / usig, sd_score); }
// Tweedie's estimate of x_0 from x_t and the score (completion.py:107, sampling.py:200): alpha, sigma^2 of return_alpha_sigma
__device__ __forceinline__ float tweedie_x0(float xt, float sigma2, float score, float alpha) { return (xt + sigma2 * score) / alpha; }
// the SNR loss weight 0.5 sqrt(1 + snr) (completion.py:143).  The one-step losses pass snr = alpha / sqrt(sigma^2) (completion.py:108), the
// multi-step loss alpha / sigma (completion.py:128): the callers form it, the two are not the same fp32 expression
__device__ __forceinline__ float snr_loss_weight(float snr) { return 0.5f * sqrtf(1.0f + snr); }
// completion imputation (sampling.py:416-420): x (1 - mask) + (mean + z std) mask, mean = mc * observation
__device__ __forceinline__ float impute(float x, float m, float obs, float mc, float z, float sd) { return x * (1.0f - m) + (mc * obs + z * sd) * m; }
template <typename T> __global__ void __launch_bounds__(256) k_em_update(WithSde<EmUpdateArgs> d) {
    const EmUpdateArgs& a = d.a;
    const int qx = a.Dpad >> 2;
    const int QD = (a.D + 3) >> 2;
    const int64_t total = a.Bpad * qx;
    // per-step scalars (identical for every sample: vec_t = ones(B)*t, sampling.py:458)
    const float t = a.t;
    const SdeAt at = sde_at(d.sde, t);
    const float mc = at.mc, sd = at.sd, beta = at.beta, g = at.g, label = at.label;
    const float usig = launch_usig(a, label);
    float mcn = 0.f, sdn = 0.f;
    if (a.t_next >= 0.f) { const SdeAt an = sde_at(d.sde, a.t_next); mcn = an.mc; sdn = an.sd; }
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s = i / qx;              // quad index fastest: row-major [B][D] streams are read/written contiguously
        const int q = (int)(i % qx);
        const int c = q * 4;
        f32x4 xn = {0.f, 0.f, 0.f, 0.f};
        if (s < a.B && c < a.D) {
            float zp[4], zb[4], za[4];
            if (a.res && !a.pf && !a.z_pred) normals4((uint64_t)s * QD + q, STREAM_EM_NOISE, a.step, a.seed, zp);   // (probability flow: none)
            if (a.obs && a.res && !a.z_impB) normals4((uint64_t)s * QD + q, STREAM_IMPUTE_B, a.step, a.seed, zb);
            if (a.obs && a.t_next >= 0.f && !a.z_impA) normals4((uint64_t)s * QD + q, STREAM_IMPUTE_A, a.step + 1, a.seed, za);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (c + r >= a.D) continue;
                const int64_t o = s * a.D + c + r;
                float x = a.x[o];
                if (a.res) {
                    // score = -(res / used_sigmas) / std                         model.py:194, utils.py:162
                    const float score = score_of_res(d.sde, a.res[s * a.Cp + c + r], usig, at.sd_score);
                    // rsde.sde: drift = -0.5 beta x - g^2 score (* 0.5 under probability flow)   sde_lib.py:98-104
                    float drift = (-0.5f * beta) * x;
                    drift = drift - ((g * g) * score) * (a.pf ? 0.5f : 1.0f);
                    const float x_mean = x + drift * d.sde.dt;                    // sampling.py:186
                    if (a.pf) {
                        x = x_mean;                                                // diffusion zeros(1): sde_lib.py:104
                    } else {
                        const float z = a.z_pred ? a.z_pred[o] : zp[r];
                        x = x_mean + (g * d.sde.sqrt_mdt) * z;                     // sampling.py:187
                    }
                    a.x_mean[o] = x_mean;
                    if (a.obs) {                                                   // sampling.py:416-420 (after predictor)
                        x = impute(x, a.mask[o], a.obs[o], mc, a.z_impB ? a.z_impB[o] : zb[r], sd);
                    }
                    if (a.traj) a.traj[o] = x;                                     // sampling.py:461
                }
                if (a.obs && a.t_next >= 0.f) {                                    // imputation ahead of the next predictor call
                    x = impute(x, a.mask[o], a.obs[o], mcn, a.z_impA ? a.z_impA[o] : za[r], sdn);
                }
                a.x[o] = x;
                xn[r] = x;
            }
        }
        store_quad_ft<T>(a.xin, s, c, a.Dpad, xn);
        if (a.x_ft) store_quad_ft<float>(a.x_ft, s, c, a.Dpad, xn);
    }
}
__global__ void __launch_bounds__(256) k_ft_to_rows(const float* a_ft, float* a, const float* b_ft, float* b, int64_t B, int D, int Dpad) {
    const int qx = Dpad >> 2;
    const int64_t total = B * qx;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s = i / qx;
        const int c = (int)(i % qx) * 4;
        const int64_t off = FT<float>::index(s, c, Dpad);
        if (a_ft) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(a_ft + off);
#pragma unroll
            for (int r = 0; r < 4; ++r) if (c + r < D) a[s * D + c + r] = v[r];
        }
        if (b_ft) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(b_ft + off);
#pragma unroll
            for (int r = 0; r < 4; ++r) if (c + r < D) b[s * D + c + r] = v[r];
        }
    }
}
hipError_t launch_ft_to_rows(const float* a_ft, float* a, const float* b_ft, float* b, int64_t B, int64_t Bpad, int D, int Dpad, hipStream_t st) {
    (void)Bpad;
    hipLaunchKernelGGL(k_ft_to_rows, dim3(grid_for(B * (Dpad >> 2))), dim3(256), 0, st, a_ft, a, b_ft, b, B, D, Dpad);
    return hipGetLastError();
}
hipError_t launch_em_update(const EmUpdateArgs& a, hipStream_t st) { return launch_quads(k_em_update<float>, k_em_update<__bf16>, a, make_sde_dev_at(a.sde, a.t), st); }

// block-wide sum -> one partial per block (deterministic)
__device__ __forceinline__ float block_sum_256(float v) {
    __shared__ float red[4];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[w] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

template <typename T> __global__ void __launch_bounds__(256) k_perturb_shared(WithSde<PerturbSharedArgs> d) {
    const PerturbSharedArgs& a = d.a;
    const int qx = a.Dpad >> 2;
    const int QD = (a.D + 3) >> 2;
    const SdeAt at = sde_at(d.sde, a.t);
    const float mc = at.mc, sd = at.sd;
    const int64_t total = a.Bpad * qx;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s = i / qx;
        const int q = (int)(i % qx);
        const int c = q * 4;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (s < a.B && c < a.D) {
            float n4[4];
            if (!a.z_in) normals4((uint64_t)s * QD + q, STREAM_PRIOR, a.step, a.seed, n4);
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (c + r < a.D) {
                    const float z = a.z_in ? a.z_in[s * a.D + c + r] : n4[r];
                    v[r] = mc * a.x0[s * a.D + c + r] + sd * z;          // completion.py:134-135
                }
        }
        store_quad_ft<T>(a.xin, s, c, a.Dpad, v);
        *reinterpret_cast<f32x4*>(a.xt + s * a.Dpad + c) = v;
    }
}
hipError_t launch_perturb_shared(const PerturbSharedArgs& a, hipStream_t st) { return launch_quads(k_perturb_shared<float>, k_perturb_shared<__bf16>, a, make_sde_dev(a.sde), st); }

__global__ void __launch_bounds__(256) k_denoise(WithSde<DenoiseArgs> d) {
    const DenoiseArgs& a = d.a;
    const SdeAt at = sde_at(d.sde, a.t);
    const float alpha = at.mc, sigma = at.sd;                         // return_alpha_sigma, sde_lib.py:227-231 (VE: 1, sigma(t), :289-292)
    const float sigma2 = sigma * sigma;
    const float usig = launch_usig(a, at.label);
    const float w = a.weighted ? snr_loss_weight(alpha / sqrtf(sigma2)) : 0.5f;     // completion.py:108,143-146
    float acc = 0.f;
    const int64_t total = a.B * a.D;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s = i / a.D;
        const int c = (int)(i % a.D);
        const float score = score_of_res(d.sde, a.res[s * a.Cp + c], usig, at.sd_score);   // (std == sigma; the DDPM table's entry for a discrete VP score function)
        const float x0h = tweedie_x0(a.xt[s * a.Dpad + c], sigma2, score, alpha);
        const float diff = a.x0[i] - x0h;
        acc += w * (diff * diff);
        if (a.x0_hat) a.x0_hat[i] = x0h;
        if (a.grad) a.grad[i] = (2.0f * w) * diff * a.inv_n;
    }
    const float tot = block_sum_256(acc);
    if (threadIdx.x == 0) a.loss_part[blockIdx.x] = tot * a.inv_n;
}
hipError_t launch_denoise(const DenoiseArgs& a, int* nblocks, hipStream_t st) {
    const WithSde<DenoiseArgs> d = {a, make_sde_dev_at(a.sde, a.t)};
    const int g = grid_for(a.B * a.D, 256, 1024);
    *nblocks = g;
    hipLaunchKernelGGL(k_denoise, dim3(g), dim3(256), 0, st, d);
    return hipGetLastError();
}

// One step of multi_step_denoise (run/completion.py:112-129, smplify.py:76-92, motion_denoising.py:106-122) behind the network evaluation at
// time_traj[i]:   noise = -score * sigma_c;   x = alpha_b / alpha_c * (x - sigma_c * noise) + sigma_b * noise
// in the reference's operation order, (alpha, sigma) = return_alpha_sigma at time_traj[i] (c) and time_traj[i + 1] (b).  The state is read
// and written as fp32 rows (xt) and re-tiled for the next GEMM (xin; padded rows / columns are zeros, as k_perturb_shared writes them).  The
// LAST step writes no state: the same pass forms x0_hat, the gradient 2 w (x0 - x0_hat) inv_n and the block partials of the loss
// (completion.py:142-147; w from the SNR alpha / sigma at time_traj[0], :127-128).
template <typename T> __global__ void __launch_bounds__(256) k_ddim_step(WithSde<DdimStepArgs> d) {
    const DdimStepArgs& a = d.a;
    const int qx = a.Dpad >> 2;
    const SdeAt at = sde_at(d.sde, a.t);
    const SdeAt ab = sde_at(d.sde, a.t_next);
    const float a_c = at.mc, s_c = at.sd, s_b = ab.sd;               // return_alpha_sigma, sde_lib.py:177-181 / :227-231 / :289-292
    const float ratio = ab.mc / a_c;
    const float usig = launch_usig(a, at.label);
    float w = 0.5f;
    if (a.last && a.weighted) {
        const SdeAt a0 = sde_at(d.sde, a.t0);
        w = snr_loss_weight(a0.mc / a0.sd);                           // completion.py:128,143
    }
    float acc = 0.f;
    const int64_t total = a.Bpad * qx;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s = i / qx;
        const int c = (int)(i % qx) * 4;
        f32x4 xn = {0.f, 0.f, 0.f, 0.f};
        if (s < a.B && c < a.D) {
            const f32x4 r4 = *reinterpret_cast<const f32x4*>(a.res + s * a.Cp + c);
            const f32x4 x4 = *reinterpret_cast<const f32x4*>(a.xt + s * a.Dpad + c);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (c + r >= a.D) continue;
                const float score = score_of_res(d.sde, r4[r], usig, at.sd_score);
                const float noise = -score * s_c;                             // completion.py:122
                const float x = ratio * (x4[r] - s_c * noise) + s_b * noise;  // :123-126
                xn[r] = x;
                if (a.last) {
                    const int64_t o = s * a.D + c + r;
                    const float diff = a.x0[o] - x;
                    acc += w * (diff * diff);
                    if (a.x0_hat) a.x0_hat[o] = x;
                    if (a.grad) a.grad[o] = (2.0f * w) * diff * a.inv_n;
                }
            }
        }
        if (!a.last) {
            store_quad_ft<T>(a.xin, s, c, a.Dpad, xn);
            *reinterpret_cast<f32x4*>(a.xt + s * a.Dpad + c) = xn;
        }
    }
    if (a.last) {
        const float tot = block_sum_256(acc);
        if (threadIdx.x == 0) a.loss_part[blockIdx.x] = tot * a.inv_n;
    }
}
hipError_t launch_ddim_step(const DdimStepArgs& a, int* nblocks, hipStream_t st) {
    const WithSde<DdimStepArgs> d = {a, make_sde_dev_at(a.sde, a.t)};
    const int g = grid_for(a.Bpad * (a.Dpad >> 2), 256, a.last ? 1024 : 8192);      // (last step: one partial per block, as k_denoise)
    *nblocks = g;
    if (a.f32) hipLaunchKernelGGL(k_ddim_step<float>, dim3(g), dim3(256), 0, st, d);
    else hipLaunchKernelGGL(k_ddim_step<__bf16>, dim3(g), dim3(256), 0, st, d);
    return hipGetLastError();
}

// One DPM-Solver++ (2M, data prediction) step behind the network evaluation at s_i (include/dposer_hip.h: dposer_dpm_sampler):
//   D_i = (x + sigma_s^2 score) / alpha_s   (k_denoise's data prediction);   x <- cx x + c0 D_i + c1 D_{i-1}
// with the three coefficients by value -- the exponential-integrator schedule is the host's, in float64; nothing here takes a log or a
// difference of log-SNRs.  D_i replaces D_{i-1} in `hist` (read only at effective order 2) and is the last step's x0_hat.  A completion
// imputes the new state at s_{i+1} in the same pass (the draw of k_em_update's look-ahead: STREAM_IMPUTE_A at step + 1).  The state leaves
// as fp32 rows and FT-tiled for the next GEMM (padded rows / columns zero, as k_perturb_shared writes them).  Each thread owns its
// elements of x / hist / x0_hat / traj, so the in-place updates need no ordering.
template <typename T> __global__ void __launch_bounds__(256) k_dpm_update(WithSde<DpmUpdateArgs> d) {
    const DpmUpdateArgs& a = d.a;
    const int qx = a.Dpad >> 2;
    const int QD = (a.D + 3) >> 2;
    const int64_t total = a.Bpad * qx;
    const SdeAt at = sde_at(d.sde, a.t);
    const float alpha = at.mc, sigma2 = at.sd * at.sd;                   // return_alpha_sigma at s_i, sde_lib.py:177-181 / :227-231 / :289-292
    const float usig = launch_usig(a, at.label);
    const bool ahead = a.obs && a.t_next >= 0.f;
    float mcn = 0.f, sdn = 0.f;
    if (ahead) { const SdeAt an = sde_at(d.sde, a.t_next); mcn = an.mc; sdn = an.sd; }
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s = i / qx;
        const int q = (int)(i % qx);
        const int c = q * 4;
        f32x4 xn = {0.f, 0.f, 0.f, 0.f};
        if (s < a.B && c < a.D) {
            const f32x4 r4 = *reinterpret_cast<const f32x4*>(a.res + s * a.Cp + c);
            float za[4];
            if (ahead && !a.z_imp) normals4((uint64_t)s * QD + q, STREAM_IMPUTE_A, a.step + 1, a.seed, za);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (c + r >= a.D) continue;
                const int64_t o = s * a.D + c + r;
                const float x0 = a.x[o];
                const float score = score_of_res(d.sde, r4[r], usig, at.sd_score);
                const float Di = tweedie_x0(x0, sigma2, score, alpha);
                float x = a.cx * x0 + a.c0 * Di;
                if (a.use_hist) x = x + a.c1 * a.hist[o];
                if (a.hist) a.hist[o] = Di;
                if (a.x0_hat) a.x0_hat[o] = Di;
                if (a.traj) a.traj[o] = x;
                if (ahead) x = impute(x, a.mask[o], a.obs[o], mcn, a.z_imp ? a.z_imp[o] : za[r], sdn);   // sampling.py:416-420 at s_{i+1}
                a.x[o] = x;
                xn[r] = x;
            }
        }
        store_quad_ft<T>(a.xin, s, c, a.Dpad, xn);
    }
}
hipError_t launch_dpm_update(const DpmUpdateArgs& a, hipStream_t st) { return launch_quads(k_dpm_update<float>, k_dpm_update<__bf16>, a, make_sde_dev_at(a.sde, a.t), st); }

// MotionDenoise.RED_Diff (run/motion_denoising.py:145-154) behind the network evaluation at x_t = mean + std z:
//   eps_pred = -score * std;   weight = sqrt(sigma^2) / alpha;   guidance = mean_b(weight * <(eps_pred - z).detach(), x_0>)
// and its gradient weight (eps_pred - z) / B w.r.t. x_0.  z is the perturbation's: the injected array, or the Philox draws of
// k_perturb_shared regenerated from the same counters.  One quad per thread, block partials in a fixed order: no float atomics.
__global__ void __launch_bounds__(256) k_red_diff(WithSde<RedDiffArgs> d) {
    const RedDiffArgs& a = d.a;
    const int QD = (a.D + 3) >> 2;
    const SdeAt at = sde_at(d.sde, a.t);
    const float alpha = at.mc, sigma = at.sd;                         // return_alpha_sigma; marginal_prob's std is the same number
    const float usig = launch_usig(a, at.label);
    const float weight = sqrtf(sigma * sigma) / alpha;                // motion_denoising.py:151-152
    float acc = 0.f;
    const int64_t total = a.B * QD;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s = i / QD;
        const int q = (int)(i % QD);
        const int c = q * 4;
        float n4[4];
        if (!a.z_in) normals4((uint64_t)s * QD + q, STREAM_PRIOR, a.step, a.seed, n4);
        const f32x4 r4 = *reinterpret_cast<const f32x4*>(a.res + s * a.Cp + c);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (c + r >= a.D) continue;
            const int64_t o = s * a.D + c + r;
            const float z = a.z_in ? a.z_in[o] : n4[r];
            const float score = score_of_res(d.sde, r4[r], usig, at.sd_score);
            const float eps = -score * sigma;                         // :150 score to noise prediction
            const float dz = eps - z;
            acc += dz * a.x0[o];
            if (a.eps_pred) a.eps_pred[o] = eps;
            if (a.grad) a.grad[o] = (weight * dz) * a.inv_batch;
        }
    }
    const float tot = block_sum_256(acc);
    if (threadIdx.x == 0) a.loss_part[blockIdx.x] = (weight * tot) * a.inv_batch;
}
hipError_t launch_red_diff(const RedDiffArgs& a, int* nblocks, hipStream_t st) {
    const WithSde<RedDiffArgs> d = {a, make_sde_dev_at(a.sde, a.t)};
    const int g = grid_for(a.B * ((a.D + 3) >> 2), 256, 1024);
    *nblocks = g;
    hipLaunchKernelGGL(k_red_diff, dim3(g), dim3(256), 0, st, d);
    return hipGetLastError();
}

// One step of DPoserComp.optimize behind the network evaluation: Tweedie estimate (completion.py:105-110), gradient of
//   w_prior * mean(w (x - x0_hat)^2) + w_data * MSE(x * mask, obs * mask)                (completion.py:131-149,195-201)
// w.r.t. x (x0_hat is detached in the reference), and torch.optim.Adam's update of x with per-element moments -- one pass
// over seven [B, D] streams instead of ~10 torch kernels.
__global__ void __launch_bounds__(256) k_completion_update(WithSde<CompletionUpdateArgs> d) {
    const CompletionUpdateArgs& a = d.a;
    const SdeAt at = sde_at(d.sde, a.t);
    const float alpha = at.mc, sigma = at.sd;                         // return_alpha_sigma, sde_lib.py:227-231
    const float sigma2 = sigma * sigma;
    const float usig = launch_usig(a, at.label);
    const float w = a.weighted ? snr_loss_weight(alpha / sqrtf(sigma2)) : 0.5f;     // completion.py:108,143-146
    const int64_t total = a.B * a.D;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s = i / a.D;
        const int c = (int)(i % a.D);
        const float score = score_of_res(d.sde, a.res[s * a.Cp + c], usig, at.sd_score);
        const float x0h = tweedie_x0(a.xt[s * a.Dpad + c], sigma2, score, alpha);
        float x = a.x[i];
        const float mk = a.mask[i];
        const float g_prior = ((2.0f * w) * (x - x0h) * a.inv_n) * a.w_prior;
        const float g_data = (((2.0f * (x * mk - a.obs[i] * mk)) * a.inv_n) * a.w_data) * mk;
        const float g = g_prior + g_data;
        float m = a.m[i], v = a.v[i];
        x = adam_step(x, g, m, v, a.s);
        a.m[i] = m;
        a.v[i] = v;
        a.x[i] = x;
    }
}
hipError_t launch_completion_update(const CompletionUpdateArgs& a, hipStream_t st) {
    const WithSde<CompletionUpdateArgs> d = {a, make_sde_dev_at(a.sde, a.t)};
    hipLaunchKernelGGL(k_completion_update, dim3(grid_for(a.B * a.D, 256, 2048)), dim3(256), 0, st, d);
    return hipGetLastError();
}

// ---- Langevin corrector (sampling.py:282-302) ------------------------------------------------------------------------
//   grad = score(x, t);  noise ~ N(0, I)
//   step = (snr * mean_b ||noise_b|| / mean_b ||grad_b||)^2 * 2 * alpha          (the means run over the WHOLE batch, :296-298)
//   x_mean = x + step * grad;   x = x_mean + sqrt(2 step) * noise
// Two passes around the grid-wide (and, under data parallelism, cross-rank) mean: norms -> [all-reduce of two scalars] -> update.
// Both recompute score and noise from the same inputs / Philox counters, so nothing but the two sums travels between them.
__global__ void __launch_bounds__(256) k_langevin_norms(WithSde<LangevinArgs> d) {
    const LangevinArgs& a = d.a;
    const int QD = (a.D + 3) >> 2;
    const SdeAt at = sde_at(d.sde, a.t);
    const float sd = at.sd_score;      // (the score's std: utils.py:155 / :160)
    const float usig = launch_usig(a, at.label);
    float gsum = 0.f, nsum = 0.f;
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < a.B; s += (int64_t)gridDim.x * blockDim.x) {
        float g2 = 0.f, n2 = 0.f;
        for (int q = 0; q < QD; ++q) {
            float z[4];
            if (!a.noise) normals4((uint64_t)s * QD + q, STREAM_LANGEVIN, a.step, a.seed, z);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int c = q * 4 + r;
                if (c >= a.D) continue;
                const float g = score_of_res(d.sde, a.res[s * a.Cp + c], usig, sd);
                const float n = a.noise ? a.noise[s * a.D + c] : z[r];
                g2 += g * g;
                n2 += n * n;
            }
        }
        gsum += sqrtf(g2);                                            // torch.norm(grad.reshape(B, -1), dim=-1)
        nsum += sqrtf(n2);
    }
    const float gt = block_sum_256(gsum);
    __syncthreads();
    const float nt = block_sum_256(nsum);
    if (threadIdx.x == 0) { a.part[blockIdx.x] = gt; a.part[gridDim.x + blockIdx.x] = nt; }
}
hipError_t launch_langevin_norms(const LangevinArgs& a, int* nblocks, hipStream_t st) {
    const WithSde<LangevinArgs> d = {a, make_sde_dev_at(a.sde, a.t)};
    const int g = grid_for(a.B, 256, 1024);
    *nblocks = g;
    hipLaunchKernelGGL(k_langevin_norms, dim3(g), dim3(256), 0, st, d);
    return hipGetLastError();
}
__global__ void __launch_bounds__(256) k_sum_partials2(const float* part, int n, float* out2) {
    float v = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) v += part[blockIdx.x * n + i];
    const float tot = block_sum_256(v);
    if (threadIdx.x == 0) out2[blockIdx.x] = tot;
}
hipError_t launch_sum_partials2(const float* part, int n, float* out2, hipStream_t st) {
    hipLaunchKernelGGL(k_sum_partials2, dim3(2), dim3(256), 0, st, part, n, out2);
    return hipGetLastError();
}
template <typename T> __global__ void __launch_bounds__(256) k_langevin_update(WithSde<LangevinArgs> d) {
    const LangevinArgs& a = d.a;
    const int qx = a.Dpad >> 2;
    const int QD = (a.D + 3) >> 2;
    const SdeAt at = sde_at(d.sde, a.t);
    const float sd = at.sd_score;      // (the score's std: utils.py:155 / :160)
    const float usig = launch_usig(a, at.label);
    const float grad_norm = a.norm_sums[0] * a.inv_global_batch, noise_norm = a.norm_sums[1] * a.inv_global_batch;   // .mean()
    const float r0 = a.snr * noise_norm / grad_norm;
    const float step = ((r0 * r0) * 2.0f) * a.alpha;                  // sampling.py:298
    const float nscale = sqrtf(step * 2.0f);                          // :300
    const int64_t total = a.Bpad * qx;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s = i / qx;
        const int q = (int)(i % qx);
        const int c = q * 4;
        f32x4 xn = {0.f, 0.f, 0.f, 0.f};
        if (s < a.B && c < a.D) {
            float z[4];
            if (!a.noise) normals4((uint64_t)s * QD + q, STREAM_LANGEVIN, a.step, a.seed, z);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (c + r >= a.D) continue;
                const int64_t o = s * a.D + c + r;
                const float g = score_of_res(d.sde, a.res[s * a.Cp + c + r], usig, sd);
                const float n = a.noise ? a.noise[o] : z[r];
                const float xm = a.x[o] + step * g;                   // :299
                const float x = xm + nscale * n;                      // :300
                a.x_mean[o] = xm;
                a.x[o] = x;
                xn[r] = x;
            }
        }
        if (a.xin) store_quad_ft<T>(a.xin, s, c, a.Dpad, xn);
    }
}
hipError_t launch_langevin_update(const LangevinArgs& a, hipStream_t st) { return launch_quads(k_langevin_update<float>, k_langevin_update<__bf16>, a, make_sde_dev_at(a.sde, a.t), st); }
// ---- predictors other than Euler-Maruyama (sampling.py:210-270) + imputation (:416-420): k_em_update's shape -----------------
// The predictor kind and the SDE kind are uniform per launch (kernel arguments): the branches in pc_pred_step do not diverge.
template <typename T> __global__ void __launch_bounds__(256) k_pc_pred_update(WithSde<PcPredArgs> d) {
    const PcPredArgs& a = d.a;
    const int qx = a.Dpad >> 2;
    const int QD = (a.D + 3) >> 2;
    const int64_t total = a.Bpad * qx;
    const SdeAt at = sde_at(d.sde, a.t);
    const float mc = at.mc, sd = at.sd;
    const float usig = launch_usig(a, at.label);
    const PcPredScal ks = pc_pred_scalars(d.sde, at, a.tab, a.pred);
    const bool score_read = a.pred != DPOSER_PC_PRED_NONE;
    const bool draws = score_read && !a.pf;
    float mcn = 0.f, sdn = 0.f;
    if (a.t_next >= 0.f) { const SdeAt an = sde_at(d.sde, a.t_next); mcn = an.mc; sdn = an.sd; }
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s = i / qx;              // quad index fastest: row-major [B][D] streams are read/written contiguously
        const int q = (int)(i % qx);
        const int c = q * 4;
        f32x4 xn = {0.f, 0.f, 0.f, 0.f};
        if (s < a.B && c < a.D) {
            float zp[4] = {0.f, 0.f, 0.f, 0.f}, zb[4], za[4];
            if (draws && !a.z_pred) normals4((uint64_t)s * QD + q, STREAM_EM_NOISE, a.step, a.seed, zp);
            if (a.obs && !a.z_impB) normals4((uint64_t)s * QD + q, STREAM_IMPUTE_B, a.step, a.seed, zb);
            if (a.obs && a.t_next >= 0.f && !a.z_impA) normals4((uint64_t)s * QD + q, STREAM_IMPUTE_A, a.step + 1, a.seed, za);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (c + r >= a.D) continue;
                const int64_t o = s * a.D + c + r;
                float x = a.x[o];
                float score = 0.f;
                if (score_read) score = score_of_res(d.sde, a.res[s * a.Cp + c + r], usig, at.sd_score);
                const float z = (draws && a.z_pred) ? a.z_pred[o] : zp[r];
                float x_mean;
                x = pc_pred_step(d.sde, a.tab, ks, a.pred, a.pf, x, score, z, &x_mean);
                a.x_mean[o] = x_mean;
                if (a.obs) {                                                   // sampling.py:416-420 (after predictor)
                    x = impute(x, a.mask[o], a.obs[o], mc, a.z_impB ? a.z_impB[o] : zb[r], sd);
                }
                if (a.traj) a.traj[o] = x;                                     // sampling.py:461
                if (a.obs && a.t_next >= 0.f) {                                // corrector 'none': imputation ahead of the next predictor call
                    x = impute(x, a.mask[o], a.obs[o], mcn, a.z_impA ? a.z_impA[o] : za[r], sdn);
                }
                a.x[o] = x;
                xn[r] = x;
            }
        }
        store_quad_ft<T>(a.xin, s, c, a.Dpad, xn);
    }
}
hipError_t launch_pc_pred_update(const PcPredArgs& a, hipStream_t st) { return launch_quads(k_pc_pred_update<float>, k_pc_pred_update<__bf16>, a, make_sde_dev_at(a.sde, a.t), st); }
// ---- annealed Langevin dynamics (sampling.py:319-339): no batch coupling, one pass; k_langevin_update's shape -------------------
template <typename T> __global__ void __launch_bounds__(256) k_ald_update(WithSde<AldArgs> d) {
    const AldArgs& a = d.a;
    const int qx = a.Dpad >> 2;
    const int QD = (a.D + 3) >> 2;
    const SdeAt at = sde_at(d.sde, a.t);
    const float usig = launch_usig(a, at.label);
    const float step = pc_ald_step_size(a.snr, at.sd, a.alpha);      // std of marginal_prob (:330), not the score's
    const float nscale = sqrtf(step * 2.0f);                          // :337
    const int64_t total = a.Bpad * qx;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s = i / qx;
        const int q = (int)(i % qx);
        const int c = q * 4;
        f32x4 xn = {0.f, 0.f, 0.f, 0.f};
        if (s < a.B && c < a.D) {
            float z[4], zi[4];
            if (!a.noise) normals4((uint64_t)s * QD + q, STREAM_LANGEVIN, a.step, a.seed, z);
            if (a.obs && !a.z_imp) normals4((uint64_t)s * QD + q, STREAM_IMPUTE_A, a.imp_step, a.seed, zi);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (c + r >= a.D) continue;
                const int64_t o = s * a.D + c + r;
                const float g = score_of_res(d.sde, a.res[s * a.Cp + c + r], usig, at.sd_score);
                const float n = a.noise ? a.noise[o] : z[r];
                const float xm = a.x[o] + step * g;                   // :336
                float x = xm + n * nscale;                            // :337
                if (a.x_mean) a.x_mean[o] = xm;
                if (a.obs) {                                          // sampling.py:416-420 (after corrector)
                    x = impute(x, a.mask[o], a.obs[o], at.mc, a.z_imp ? a.z_imp[o] : zi[r], at.sd);
                }
                a.x[o] = x;
                xn[r] = x;
            }
        }
        store_quad_ft<T>(a.xin, s, c, a.Dpad, xn);
    }
}
hipError_t launch_ald_update(const AldArgs& a, hipStream_t st) { return launch_quads(k_ald_update<float>, k_ald_update<__bf16>, a, make_sde_dev_at(a.sde, a.t), st); }
// row-major [B][D] fp32 -> FT [Bpad][Dpad] network input (zero padded)
// ---- MCG / DPS guided Euler-Maruyama step (sampling.py:191-207 around RSDE.sde(guide=True), sde_lib.py:98-109) -------------------------
//   y0 = (x + sigma^2 score) / alpha;  r = obs mask - y0 mask;  norm = ||r||_F over the WHOLE batch (:201)
//   grad = d norm / d x = u / alpha + J_score^T [(sigma^2 / alpha) u],  u = -mask r / norm
//   x = y_mean + g sqrt(-dt) z - grad_step grad;  x_mean = y_mean;  MCG: the imputation of :416-420 behind it
// Two passes around the grid-wide norm and the network's dgrad: `resid` writes the upstream gradient of the backward WITHOUT the 1 / norm
// (the backward is linear in it) and the partial sums of r^2; `update` recomputes score and r from the same inputs, divides by the norm and
// steps.  k_langevin_norms / k_langevin_update's shape.
struct GuidedScal { float mc, sd, sd2, beta, g, sds, usig; };
template <typename A> __device__ __forceinline__ GuidedScal guided_scalars(const A& a, const SdeDev& sde) {
    const SdeAt at = sde_at(sde, a.t);
    GuidedScal k;
    k.mc = at.mc; k.sd = at.sd; k.sd2 = at.sd * at.sd; k.beta = at.beta; k.g = at.g; k.sds = at.sd_score;   // return_alpha_sigma: alpha = mc, sigma = std
    k.usig = launch_usig(a, at.label);
    return k;
}
// r = obs mask - y0 mask and the score, for one element
__device__ __forceinline__ float guided_resid(const SdeDev& sde, const GuidedScal& k, float res, float x, float obs, float m, float* score_out) {
    const float score = score_of_res(sde, res, k.usig, k.sds);
    const float y0 = tweedie_x0(x, k.sd2, score, k.mc);                             // sampling.py:200
    *score_out = score;
    return obs * m - y0 * m;                                                        // :201
}
template <typename T> __global__ void __launch_bounds__(256) k_guided_resid(WithSde<GuidedArgs> d) {
    const GuidedArgs& a = d.a;
    const int qc = a.Cp >> 2;
    const int64_t total = a.Bpad * qc;
    const GuidedScal k = guided_scalars(a, d.sde);
    float acc = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s = i / qc;
        const int c = (int)(i % qc) * 4;
        f32x4 dr = {0.f, 0.f, 0.f, 0.f};
        if (s < a.B && c < a.D) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (c + r >= a.D) continue;
                const int64_t o = s * a.D + c + r;
                const float m = a.mask[o];
                float score;
                const float rr = guided_resid(d.sde, k, a.res[s * a.Cp + c + r], a.x[o], a.obs[o], m, &score);
                acc += rr * rr;
                // autograd of the norm's argument down to res, without the 1 / norm: d / d y0 = -mask r, / alpha, * sigma^2 (the score's share),
                // d score / d model (sde_score), / used_sigmas
                const float gscore = ((-(m * rr)) / k.mc) * k.sd2;
                const float gmodel = d.sde.kind == SDE_VE ? gscore : -(gscore / k.sds);
                dr[r] = gmodel / k.usig;
            }
        }
        store_quad_ft<T>(a.dres, s, c, a.Cp, dr);
    }
    const float tot = block_sum_256(acc);
    if (threadIdx.x == 0) a.part[blockIdx.x] = tot;
}
hipError_t launch_guided_resid(const GuidedArgs& a, int* nblocks, hipStream_t st) {
    const WithSde<GuidedArgs> d = {a, make_sde_dev_at(a.sde, a.t)};
    const int g = grid_for(a.Bpad * (a.Cp >> 2), 256, 1024);
    *nblocks = g;
    hipLaunchKernelGGL(a.f32 ? k_guided_resid<float> : k_guided_resid<__bf16>, dim3(g), dim3(256), 0, st, d);
    return hipGetLastError();
}
template <typename T> __global__ void __launch_bounds__(256) k_guided_update(WithSde<GuidedArgs> d) {
    const GuidedArgs& a = d.a;
    const int qx = a.Dpad >> 2;
    const int QD = (a.D + 3) >> 2;
    const int64_t total = a.Bpad * qx;
    const GuidedScal k = guided_scalars(a, d.sde);
    const float norm = sqrtf(a.norm_sq[0]);                                         // torch.norm: the square root of the sum of squares
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s = i / qx;              // quad index fastest: row-major [B][D] streams are read/written contiguously
        const int q = (int)(i % qx);
        const int c = q * 4;
        f32x4 xn = {0.f, 0.f, 0.f, 0.f};
        if (s < a.B && c < a.D) {
            float zp[4], zi[4];
            if (!a.z_pred) normals4((uint64_t)s * QD + q, STREAM_EM_NOISE, a.step, a.seed, zp);
            if (a.project && !a.z_imp) normals4((uint64_t)s * QD + q, STREAM_IMPUTE_B, a.step, a.seed, zi);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (c + r >= a.D) continue;
                const int64_t o = s * a.D + c + r;
                const float x0 = a.x[o], m = a.mask[o], obs = a.obs[o];
                float score;
                const float rr = guided_resid(d.sde, k, a.res[s * a.Cp + c + r], x0, obs, m, &score);
                // rsde.sde: drift = -0.5 beta x - g^2 score                           sde_lib.py:98-104
                float drift = (-0.5f * k.beta) * x0;
                drift = drift - (k.g * k.g) * score;
                const float y_mean = x0 + drift * d.sde.dt;                            // sampling.py:196
                const float y_hat = y_mean + (k.g * d.sde.sqrt_mdt) * (a.z_pred ? a.z_pred[o] : zp[r]);   // :197
                // d norm / d x: the direct share of y0 and the network's, both still times norm; norm == 0: torch's norm backward gives 0
                const float gn = (-(m * rr)) / k.mc + a.dx[o];
                const float grad = norm == 0.0f ? 0.0f : gn / norm;
                if (!isfinite(grad)) bad = true;                                       // :203-204
                float x = y_hat - a.grad_step * grad;                                  // :205
                a.x_mean[o] = y_mean;
                if (a.project) x = impute(x, m, obs, k.mc, a.z_imp ? a.z_imp[o] : zi[r], k.sd);   // :416-420
                if (a.traj) a.traj[o] = x;
                a.x[o] = x;
                xn[r] = x;
            }
        }
        store_quad_ft<T>(a.xin, s, c, a.Dpad, xn);
    }
    if (bad) atomicMin(a.nonfinite, (int32_t)a.step);
}
hipError_t launch_guided_update(const GuidedArgs& a, hipStream_t st) { return launch_quads(k_guided_update<float>, k_guided_update<__bf16>, a, make_sde_dev_at(a.sde, a.t), st); }

// ---- DPS on observed 3D joints (dposer_joint_guided_sampler): the guided step above with the joint-residual stage of jointguide.hip as the
// measurement.  norm = sqrt(s) with s = sum_live c |J(denormalise(y0)) - o|^2 (per row, or summed over the batch), d norm / d y0 = v / norm with
// v = 1/2 d s / d y0 -- so v stands where k_guided_resid / k_guided_update form -mask r, and three passes stand around the stage and the dgrad:
//   y0      the Tweedie estimate as fp32 rows for the stage
//   dres    the upstream gradient of the backward from the stage's v, WITHOUT the 1 / norm (the backward is linear in it)
//   update  k_guided_update reading the stored v and s where that kernel recomputes its residual
__global__ void __launch_bounds__(256) k_joint_guided_y0(WithSde<JointGuidedArgs> d) {
    const JointGuidedArgs& a = d.a;
    const GuidedScal k = guided_scalars(a, d.sde);
    const int64_t total = a.B * a.D;
    for (int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s = o / a.D;
        const int c = (int)(o % a.D);
        const float score = score_of_res(d.sde, a.res[s * a.Cp + c], k.usig, k.sds);
        a.y0[o] = tweedie_x0(a.x[o], k.sd2, score, k.mc);                              // sampling.py:200
    }
}
hipError_t launch_joint_guided_y0(const JointGuidedArgs& a, hipStream_t st) {
    const WithSde<JointGuidedArgs> d = {a, make_sde_dev_at(a.sde, a.t)};
    hipLaunchKernelGGL(k_joint_guided_y0, dim3(grid_for(a.B * a.D)), dim3(256), 0, st, d);
    return hipGetLastError();
}
template <typename T> __global__ void __launch_bounds__(256) k_joint_guided_dres(WithSde<JointGuidedArgs> d) {
    const JointGuidedArgs& a = d.a;
    const int qc = a.Cp >> 2;
    const int64_t total = a.Bpad * qc;
    const GuidedScal k = guided_scalars(a, d.sde);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s = i / qc;
        const int c = (int)(i % qc) * 4;
        f32x4 dr = {0.f, 0.f, 0.f, 0.f};
        if (s < a.B && c < a.D) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (c + r >= a.D) continue;
                // k_guided_resid's chain with v for -mask r: / alpha, * sigma^2 (the score's share), d score / d model, / used_sigmas
                const float gscore = (a.v[s * a.D + c + r] / k.mc) * k.sd2;
                const float gmodel = d.sde.kind == SDE_VE ? gscore : -(gscore / k.sds);
                dr[r] = gmodel / k.usig;
            }
        }
        store_quad_ft<T>(a.dres, s, c, a.Cp, dr);
    }
}
hipError_t launch_joint_guided_dres(const JointGuidedArgs& a, hipStream_t st) {
    const WithSde<JointGuidedArgs> d = {a, make_sde_dev_at(a.sde, a.t)};
    hipLaunchKernelGGL(a.f32 ? k_joint_guided_dres<float> : k_joint_guided_dres<__bf16>, dim3(grid_for(a.Bpad * (a.Cp >> 2), 256, 1024)), dim3(256), 0, st, d);
    return hipGetLastError();
}
template <typename T> __global__ void __launch_bounds__(256) k_joint_guided_update(WithSde<JointGuidedArgs> d) {
    const JointGuidedArgs& a = d.a;
    const int qx = a.Dpad >> 2;
    const int QD = (a.D + 3) >> 2;
    const int64_t total = a.Bpad * qx;
    const GuidedScal k = guided_scalars(a, d.sde);
    const float norm_batch = a.norm_scope == 0 ? sqrtf(a.norm_sq[0]) : 0.f;            // torch.norm over the whole tensor (sampling.py:201)
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s = i / qx;
        const int q = (int)(i % qx);
        const int c = q * 4;
        f32x4 xn = {0.f, 0.f, 0.f, 0.f};
        if (s < a.B && c < a.D) {
            float zp[4];
            if (!a.z_pred) normals4((uint64_t)s * QD + q, STREAM_EM_NOISE, a.step, a.seed, zp);
            const float norm = a.norm_scope == 0 ? norm_batch : sqrtf(a.s[s]);          // "sample": every row is its own problem
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (c + r >= a.D) continue;
                const int64_t o = s * a.D + c + r;
                const float x0 = a.x[o];
                const float score = score_of_res(d.sde, a.res[s * a.Cp + c + r], k.usig, k.sds);
                float drift = (-0.5f * k.beta) * x0;                                   // sde_lib.py:98-104
                drift = drift - (k.g * k.g) * score;
                const float y_mean = x0 + drift * d.sde.dt;                            // sampling.py:196
                const float y_hat = y_mean + (k.g * d.sde.sqrt_mdt) * (a.z_pred ? a.z_pred[o] : zp[r]);   // :197
                // d norm / d x times norm: y0's direct share and the network's; norm == 0 (no live entry, or an exact fit): no guidance
                const float gn = a.v[o] / k.mc + a.dx[o];
                const float grad = norm == 0.0f ? 0.0f : gn / norm;
                if (!isfinite(grad)) bad = true;                                       // :203-204
                const float x = y_hat - a.grad_step * grad;                            // :205
                a.x_mean[o] = y_mean;
                if (a.traj) a.traj[o] = x;
                a.x[o] = x;
                xn[r] = x;
            }
        }
        store_quad_ft<T>(a.xin, s, c, a.Dpad, xn);
    }
    if (bad) atomicMin(a.nonfinite, (int32_t)a.step);
}
hipError_t launch_joint_guided_update(const JointGuidedArgs& a, hipStream_t st) {
    return launch_quads(k_joint_guided_update<float>, k_joint_guided_update<__bf16>, a, make_sde_dev_at(a.sde, a.t), st);
}

template <typename T> __global__ void __launch_bounds__(256) k_pack_rows(const float* x, void* xin, int64_t B, int64_t Bpad, int D, int Dpad) {
    const int qx = Dpad >> 2;
    const int64_t total = Bpad * qx;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s = i / qx;
        const int c = (int)(i % qx) * 4;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (s < B)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (c + r < D) v[r] = x[s * D + c + r];
        store_quad_ft<T>(xin, s, c, Dpad, v);
    }
}
hipError_t launch_pack_rows(const float* x, void* xin, int64_t B, int64_t Bpad, int D, int Dpad, int f32, hipStream_t st) {
    const int64_t total = Bpad * (Dpad >> 2);
    if (f32) hipLaunchKernelGGL(k_pack_rows<float>, dim3(grid_for(total)), dim3(256), 0, st, x, xin, B, Bpad, D, Dpad);
    else hipLaunchKernelGGL(k_pack_rows<__bf16>, dim3(grid_for(total)), dim3(256), 0, st, x, xin, B, Bpad, D, Dpad);
    return hipGetLastError();
}

// One thread keeps ONE channel quad q for all of its samples (thread t: q = t % qc, sample lane t / qc; 256 / qc sample lanes per block),
// so that the column sums of dres -- the gradient of post_dense's bias, a k_colsum launch of its own before -- are per-thread running sums:
// each block leaves one partial row [Cp] (fixed order: sample lanes in turn), the last reduction of the step adds the rows.
template <typename T> __global__ void __launch_bounds__(256) k_dsm(WithSde<DsmArgs> d) {
    __shared__ float cs[256][4];
    const DsmArgs& a = d.a;
    const int qc = a.Cp >> 2;
    const int lanes = 256 / qc;                       // sample lanes of the block (Cp <= 512: >= 2)
    const int q = threadIdx.x % qc, sl = threadIdx.x / qc;
    const int c = q * 4;
    float acc = 0.f;
    f32x4 csum = {0.f, 0.f, 0.f, 0.f};
    if (sl < lanes) {
        for (int64_t s = (int64_t)blockIdx.x * lanes + sl; s < a.Bpad; s += (int64_t)gridDim.x * lanes) {
            f32x4 dr = {0.f, 0.f, 0.f, 0.f};
            if (s < a.B && c < a.D) {
                const float t = a.t[s];
                const SdeAt at = sde_at(d.sde, t);
                const float sd = at.sd;
                const float usig = a.scale_by_sigma ? used_sigma(a.sigmas, a.num_scales, at.label, a.fourier) : 1.0f;
                const bool ve = d.sde.kind == SDE_VE;
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (c + r < a.D) {
                        const float model = a.res[s * a.Cp + c + r] / usig;
                        const float score = sde_score(d.sde, model, sd);               // utils.py:162 / :180
                        const float e = score * sd + a.z[s * a.Dpad + c + r];          // losses.py:124
                        acc += e * e;
                        // d e / d res = -1 / used_sigma (sub-VP / VP: std cancels) or std / used_sigma (VE)
                        dr[r] = ve ? ((2.0f * e) * sd) * a.grad_scale / usig : (-2.0f * e) * a.grad_scale / usig;
                    }
            }
            store_quad_ft<T>(a.dres, s, c, a.Cp, dr);
            // the bias gradient sums what the GEMMs read: the stored (bf16-rounded in bf16 mode) values, like k_colsum did
            const f32x4 st4 = Quad<T>::round_trip(dr);
#pragma unroll
            for (int r = 0; r < 4; ++r) csum[r] += st4[r];
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) cs[threadIdx.x][r] = csum[r];
    const float tot = block_sum_256(acc);             // (contains the barrier that publishes cs)
    if (threadIdx.x == 0) a.loss_part[blockIdx.x] = tot * a.grad_scale;
    if (a.cs_part && threadIdx.x < qc) {
        f32x4 t4 = {0.f, 0.f, 0.f, 0.f};
        for (int l = 0; l < lanes; ++l)
#pragma unroll
            for (int r = 0; r < 4; ++r) t4[r] += cs[l * qc + threadIdx.x][r];
        *reinterpret_cast<f32x4*>(a.cs_part + (int64_t)blockIdx.x * a.Cp + c) = t4;
    }
}
hipError_t launch_dsm(const DsmArgs& a, int* nblocks, hipStream_t st) {
    const WithSde<DsmArgs> d = {a, make_sde_dev(a.sde)};
    const int lanes = 256 / (a.Cp >> 2);
    int64_t g = (a.Bpad + lanes - 1) / lanes;
    g = g < 1 ? 1 : (g > 1024 ? 1024 : g);
    *nblocks = (int)g;
    if (a.f32) hipLaunchKernelGGL(k_dsm<float>, dim3((unsigned)g), dim3(256), 0, st, d);
    else hipLaunchKernelGGL(k_dsm<__bf16>, dim3((unsigned)g), dim3(256), 0, st, d);
    return hipGetLastError();
}

// The time-branch dgrad at small batches (a few dozen 128 x 128 tiles with K = L * H): the GEMM runs as one k-split per layer segment
// (EpiPartialFT), this kernel adds the splits in order, applies act'(u) and keeps the column sums of the stored dU (the shared
// embedding's bias gradient), like the one-launch epilogue (EpiSiLUBwd) does.  A thread keeps ONE channel quad for all of its samples.
template <typename T> __global__ void __launch_bounds__(256) k_silu_bwd_reduce(SiLUBwdReduceArgs a) {
    __shared__ float cs[256][4];
    constexpr bool PRECISE = sizeof(T) == 4;
    constexpr int MAXS = 8, SPT = 4;                  // splits held in registers / samples per thread and pass (all loads of a pass in flight)
    const int qc = a.N >> 2;                          // quads per sample row (N <= 1024: qc <= 256)
    const int lanes = 256 / qc;
    const int q = threadIdx.x % qc, sl = threadIdx.x / qc;
    const int c = q * 4;
    f32x4 csum = {0.f, 0.f, 0.f, 0.f};
    if (sl < lanes) {
        const int64_t step = (int64_t)gridDim.x * lanes;
        for (int64_t s0 = (int64_t)blockIdx.x * lanes + sl; s0 < a.Spad; s0 += step * SPT) {
            f32x4 part[SPT][MAXS], u[SPT];
#pragma unroll
            for (int i = 0; i < SPT; ++i) {
                const int64_t s = s0 + i * step;
                const bool live = s < a.B;
                const int64_t idx = live ? FT<float>::index(s, c, a.N) : 0;
#pragma unroll
                for (int k = 0; k < MAXS; ++k)
                    part[i][k] = (live && k < a.nsplit) ? Quad<float>::load(a.part + (int64_t)k * a.split_stride + idx) : f32x4{0.f, 0.f, 0.f, 0.f};
                u[i] = live ? Quad<T>::load(reinterpret_cast<const T*>(a.pre) + FT<T>::index(s, c, a.N)) : f32x4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int i = 0; i < SPT; ++i) {
                const int64_t s = s0 + i * step;
                if (s >= a.Spad) break;
                f32x4 acc = part[i][0];
#pragma unroll
                for (int k = 1; k < MAXS; ++k)                // in split (= layer) order; absent splits add +0
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[r] += part[i][k][r];
                f32x4 o = {0.f, 0.f, 0.f, 0.f};
                if (s < a.B) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) o[r] = acc[r] * (a.act == DP_ACT_SWISH ? dsilu_f<PRECISE>(u[i][r]) : dact_rt<PRECISE>(u[i][r], a.act));
                }
                store_quad_ft<T>(a.out, s, c, a.N, o);
                const f32x4 st4 = Quad<T>::round_trip(o);
#pragma unroll
                for (int r = 0; r < 4; ++r) csum[r] += st4[r];
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) cs[threadIdx.x][r] = csum[r];
    __syncthreads();
    if (threadIdx.x < qc) {
        f32x4 t4 = {0.f, 0.f, 0.f, 0.f};
        for (int l = 0; l < lanes; ++l)
#pragma unroll
            for (int r = 0; r < 4; ++r) t4[r] += cs[l * qc + threadIdx.x][r];
        *reinterpret_cast<f32x4*>(a.cs_part + (int64_t)blockIdx.x * a.N + c) = t4;
    }
}
hipError_t launch_silu_bwd_reduce(const SiLUBwdReduceArgs& a, int max_blocks, int* nblocks, hipStream_t st) {
    if (a.N % 4 != 0 || a.N > 1024) return hipErrorInvalidValue;
    if (a.nsplit < 1 || a.nsplit > 8) return hipErrorInvalidValue;
    const int lanes = 256 / (a.N >> 2);
    int64_t g = (a.Spad + lanes * 4 - 1) / (lanes * 4);      // four samples per thread: a quarter of the rows for the final reduction
    g = g < 1 ? 1 : (g > max_blocks ? max_blocks : g);
    *nblocks = (int)g;
    if (a.f32) hipLaunchKernelGGL(k_silu_bwd_reduce<float>, dim3((unsigned)g), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_silu_bwd_reduce<__bf16>, dim3((unsigned)g), dim3(256), 0, st, a);
    return hipGetLastError();
}

// FT-order form (fp32 storage): block (x, y) owns the four k-blocks [4 x, 4 x + 4) -- 32 columns -- of the row blocks y, y + gridDim.y, ...;
// thread = (k-block, lane) keeps ONE column quad for all of its rows, so its column sums stay in registers; the 32 lanes (rows) of a
// (k-block, half) are added through LDS at the end, in lane order.  Same per-element arithmetic and split order as k_silu_bwd_reduce.
__global__ void __launch_bounds__(256) k_silu_bwd_reduce_ft(SiLUBwdReduceArgs a, __bf16* __restrict__ out_hi, __bf16* __restrict__ out_lo) {
    __shared__ float cs[256][4];
    const int kbs = a.N >> 3;                                       // FT32 k-blocks per row block
    const int kb = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, kh = lane >> 5, r = lane & 31;
    const int c = 8 * kb + 4 * kh;
    f32x4 csum = {0.f, 0.f, 0.f, 0.f};
    const float* pre = reinterpret_cast<const float*>(a.pre);
    float* out = reinterpret_cast<float*>(a.out);
    for (int64_t rb = blockIdx.y; rb < (a.Spad >> 5); rb += gridDim.y) {
        const int64_t idx = ((rb * kbs + kb) << 8) + lane * 4;      // this thread's chunk of FT32 block (rb, kb)
        const bool live = rb * 32 + r < a.B;
        f32x4 acc = *reinterpret_cast<const f32x4*>(a.part + idx);
        for (int k = 1; k < a.nsplit; ++k) {                        // in split (= layer) order
            const f32x4 v = *reinterpret_cast<const f32x4*>(a.part + (int64_t)k * a.split_stride + idx);
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] += v[q];
        }
        const f32x4 u = *reinterpret_cast<const f32x4*>(pre + idx);
        f32x4 o = {0.f, 0.f, 0.f, 0.f};
        if (live) {
#pragma unroll
            for (int q = 0; q < 4; ++q) o[q] = acc[q] * (a.act == DP_ACT_SWISH ? dsilu_f<true>(u[q]) : dact_rt<true>(u[q], a.act));
        }
        *reinterpret_cast<f32x4*>(out + idx) = o;
        if (out_hi) {      // this thread's half (kh) of the 16-byte chunk of FT16 block (rb, kb >> 1), lane ((kb & 1), r)
            __bf16 h4[4], l4[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) { h4[q] = (__bf16)o[q]; l4[q] = (__bf16)(o[q] - (float)h4[q]); }
            const int64_t pidx = (((rb * (a.N >> 4) + (kb >> 1)) << 6) + ((kb & 1) << 5) + r) * 8 + kh * 4;
            *reinterpret_cast<uint2*>(out_hi + pidx) = *reinterpret_cast<const uint2*>(h4);
            *reinterpret_cast<uint2*>(out_lo + pidx) = *reinterpret_cast<const uint2*>(l4);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) csum[q] += o[q];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) cs[threadIdx.x][q] = csum[q];
    __syncthreads();
    if (r == 0) {                                                   // 8 threads: one per (k-block, half)
        f32x4 t4 = {0.f, 0.f, 0.f, 0.f};
        for (int l = 0; l < 32; ++l)
#pragma unroll
            for (int q = 0; q < 4; ++q) t4[q] += cs[threadIdx.x + l][q];
        *reinterpret_cast<f32x4*>(a.cs_part + (int64_t)blockIdx.y * a.N + c) = t4;
    }
}
hipError_t launch_silu_bwd_reduce_ft(const SiLUBwdReduceArgs& a, void* out_hi, void* out_lo, int max_blocks, int* nblocks, hipStream_t st) {
    if (a.N % 32 != 0 || !a.f32 || a.nsplit < 1) return hipErrorInvalidValue;
    int64_t gy = a.Spad >> 5;
    gy = gy > 256 ? 256 : gy;                                        // partial rows of column sums (each block walks Spad / 32 / gy row blocks)
    gy = gy > max_blocks ? max_blocks : gy;
    *nblocks = (int)gy;
    hipLaunchKernelGGL(k_silu_bwd_reduce_ft, dim3((unsigned)(a.N / 32), (unsigned)gy), dim3(256), 0, st, a, (__bf16*)out_hi, (__bf16*)out_lo);
    return hipGetLastError();
}

template <typename T> __global__ void __launch_bounds__(256) k_dres_from_dout(DresArgs a) {
    const int qc = a.Cp >> 2;
    const int64_t total = a.Bpad * qc;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s = i / qc;
        const int c = (int)(i % qc) * 4;
        f32x4 dr = {0.f, 0.f, 0.f, 0.f};
        if (s < a.B && c < a.D) {
            const float usig = a.scale_by_sigma ? used_sigma(a.sigmas, a.num_scales, a.labels[s], a.fourier) : 1.0f;
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (c + r < a.D) dr[r] = a.dout[s * a.D + c + r] / usig;
        }
        store_quad_ft<T>(a.dres, s, c, a.Cp, dr);
    }
}
hipError_t launch_dres_from_dout(const DresArgs& a, hipStream_t st) {
    const int64_t total = a.Bpad * (a.Cp >> 2);
    if (a.f32) hipLaunchKernelGGL(k_dres_from_dout<float>, dim3(grid_for(total)), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_dres_from_dout<__bf16>, dim3(grid_for(total)), dim3(256), 0, st, a);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// layout helpers
// ------------------------------------------------------------------------------------------------
// One block transposes a 32-sample x 32-channel tile through LDS.
template <typename T> __global__ void __launch_bounds__(256) k_ft_transpose(const T* in, T* out, int64_t Spad, int C, int Cpad) {
    __shared__ float tile[32][33];
    const int64_t s0 = (int64_t)blockIdx.x * 32;
    const int c0 = blockIdx.y * 32;
    {
        const int sl = threadIdx.x & 31, cq = threadIdx.x >> 5;          // 8 channel quads
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (c0 + cq * 4 < C) v = Quad<T>::load(in + FT<T>::index(s0 + sl, c0 + cq * 4, C));
#pragma unroll
        for (int r = 0; r < 4; ++r) tile[cq * 4 + r][sl] = v[r];
    }
    __syncthreads();
    {
        const int cl = threadIdx.x & 31, sq = threadIdx.x >> 5;          // 8 sample quads
        f32x4 v;
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = tile[cl][sq * 4 + r];
        Quad<T>::store(out + FT<T>::index(c0 + cl, (int)(s0 + sq * 4), (int)Spad), v);
    }
}
hipError_t launch_ft_transpose(int f32, const void* in, void* out, int64_t Spad, int C, hipStream_t st) {
    const int Cpad = (int)round_up(C, 32);
    dim3 grid((unsigned)(Spad / 32), (unsigned)(Cpad / 32));
    if (f32) hipLaunchKernelGGL(k_ft_transpose<float>, grid, dim3(256), 0, st, (const float*)in, (float*)out, Spad, C, Cpad);
    else hipLaunchKernelGGL(k_ft_transpose<__bf16>, grid, dim3(256), 0, st, (const __bf16*)in, (__bf16*)out, Spad, C, Cpad);
    return hipGetLastError();
}

// ---- bf16 x 3 precision mode: an fp32 fragment-tiled matrix as two bf16 fragment-tiled planes ------------------------------------------
// x = hi + lo + O(2^-17 |x|), hi = bf16(x), lo = bf16(x - hi): the operands of the three-term products hi*hi + lo*hi + hi*lo that the
// bf16 matrix pipe accumulates in fp32 (scorefc.hip, precision DPOSER_PREC_BF16X3; the LBS blend GEMMs use the same split, fk.hip).
// FT32 block (rb, kb): lane (kh, r) holds T[32 rb + r][8 kb + 4 kh + 0..3]; FT16 block (rb, kb'): lane (kh, r) holds
// T[32 rb + r][16 kb' + 8 kh + 0..7] = the two lane halves' chunks of FT32 block (rb, 2 kb' + kh).  One thread = one 16-byte output chunk
// per plane: two 16-byte reads (512 B apart, each a coalesced 512-B run per half-wave), two 16-byte writes (1 KiB runs).
__global__ void __launch_bounds__(256) k_split_ft32(const float* __restrict__ src, __bf16* __restrict__ hi, __bf16* __restrict__ lo, int64_t n_chunks) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;           // output chunk: block (i >> 6), lane (i & 63)
    if (i >= n_chunks) return;
    const int64_t blk = i >> 6;
    const int lane = (int)(i & 63), kh = lane >> 5, r = lane & 31;
    const float* s = src + ((2 * blk + kh) << 8);                         // FT32 block (rb, 2 kb' + kh): 256 floats; (rb * K/16 + kb') * 2 + kh
    const f32x4 a = *reinterpret_cast<const f32x4*>(s + r * 4), b = *reinterpret_cast<const f32x4*>(s + (32 + r) * 4);
    const float v[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    __bf16 h8[8], l8[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        h8[e] = (__bf16)v[e];
        l8[e] = (__bf16)(v[e] - (float)h8[e]);
    }
    *reinterpret_cast<u32x4*>(hi + i * 8) = *reinterpret_cast<const u32x4*>(h8);
    *reinterpret_cast<u32x4*>(lo + i * 8) = *reinterpret_cast<const u32x4*>(l8);
}
hipError_t launch_split_ft32(const void* src, void* hi, void* lo, int64_t rows_pad, int K, hipStream_t st) {
    const int64_t n_chunks = rows_pad * (int64_t)K / 8;                  // (rows_pad % 32 == 0, K % 16 == 0: whole FT16 blocks)
    hipLaunchKernelGGL(k_split_ft32, dim3((unsigned)((n_chunks + 255) / 256)), dim3(256), 0, st, (const float*)src, (__bf16*)hi, (__bf16*)lo, n_chunks);
    return hipGetLastError();
}

constexpr int COLSUM_CHUNK = 2048;   // samples per partial row
template <typename T> __global__ void __launch_bounds__(256) k_colsum(const T* in, float* part, int64_t Spad, int C, SumJob sj) {
    if (blockIdx.y == gridDim.y - 1 && sj.n > 0) {      // rider: out[0] = sum(part[0..n)) -- k_sum_partials' order, one launch less
        if (blockIdx.x == 0) {
            float acc = 0.f;
            for (int i = threadIdx.x; i < sj.n; i += 256) acc += sj.part[i];
            const float tot = block_sum_256(acc);
            if (threadIdx.x == 0) sj.out[0] = tot;
        }
        return;
    }
    // block = (channel quad group of 8 quads, sample chunk): thread (sl = tid&31, cq = tid>>5)
    const int c = (blockIdx.x * 8 + (threadIdx.x >> 5)) * 4;
    const int64_t s_begin = (int64_t)blockIdx.y * COLSUM_CHUNK;
    const int64_t s_end = s_begin + COLSUM_CHUNK < Spad ? s_begin + COLSUM_CHUNK : Spad;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (c < C) {
        // 8 loads in flight per thread, added in sample order (same summation order as a plain loop; one load per trip
        // is a chain of 64 dependent L2 / HBM round trips: 28 us per call at 8192 samples)
        int64_t s = s_begin + (threadIdx.x & 31);
        for (; s + 7 * 32 < s_end; s += 8 * 32) {
            f32x4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = Quad<T>::load(in + FT<T>::index(s + u * 32, c, C));
#pragma unroll
            for (int u = 0; u < 8; ++u)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[r] += v[u][r];
        }
        for (; s < s_end; s += 32) {
            f32x4 v = Quad<T>::load(in + FT<T>::index(s, c, C));
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[r] += v[r];
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int d = 16; d >= 1; d >>= 1) acc[r] += __shfl_xor(acc[r], d);
    if ((threadIdx.x & 31) == 0 && c < C) {
#pragma unroll
        for (int r = 0; r < 4; ++r) part[(int64_t)blockIdx.y * C + c + r] = acc[r];
    }
}
hipError_t launch_colsum(int f32, const void* in, float* part, int64_t Spad, int C, int* nchunks, hipStream_t st, const SumJob* rider) {
    const int nc = (int)ceil_div(Spad, COLSUM_CHUNK);
    *nchunks = nc;
    SumJob sj{nullptr, 0, nullptr};
    if (rider && rider->n > 0) sj = *rider;
    dim3 grid((unsigned)ceil_div(C / 4, 8), (unsigned)(nc + (sj.n > 0 ? 1 : 0)));
    if (f32) hipLaunchKernelGGL(k_colsum<float>, grid, dim3(256), 0, st, (const float*)in, part, Spad, C, sj);
    else hipLaunchKernelGGL(k_colsum<__bf16>, grid, dim3(256), 0, st, (const __bf16*)in, part, Spad, C, sj);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// gradient finalisation and optimizer
// ------------------------------------------------------------------------------------------------
// one job of the deterministic reductions into the flat gradient; (bx, nbx): this block's index / the number of blocks of the job
__device__ __forceinline__ void reduce_job_body(const ReduceJob& j, const float* scratch, float* grad, int bx, int nbx, float (*red)[32], float* alt) {
    if (j.nsrc < 0) {       // plain sum of a list of partials to a scalar outside the gradient (k_sum_partials' order; one block)
        if (bx == 0) {
            float acc = 0.f;
            for (int i = threadIdx.x; i < (int)j.count; i += 256) acc += scratch[j.src_off + i];
            const float tot = block_sum_256(acc);
            if (threadIdx.x == 0) alt[0] = tot;
        }
        return;
    }
    if (j.nsrc == 0) {      // a range that never gets a gradient (dead parameters): zeros -- was a memset launch of its own
        const bool al = ((j.dst_off | j.count) & 3) == 0;
        const int64_t n4 = al ? (j.count >> 2) : 0;
        for (int64_t e = (int64_t)bx * 256 + threadIdx.x; e < n4; e += (int64_t)nbx * 256)
            reinterpret_cast<f32x4*>(grad + j.dst_off)[e] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int64_t e = (n4 << 2) + (int64_t)bx * 256 + threadIdx.x; e < j.count; e += (int64_t)nbx * 256)
            grad[j.dst_off + e] = 0.f;
        return;
    }
    if (j.nsrc > 64) {
        // many partial rows, few elements (GroupNorm / bias partials): 32 elements x 8 source slices per block,
        // fixed summation order => deterministic
        const int el = threadIdx.x & 31, sl = threadIdx.x >> 5;
        for (int64_t e0 = (int64_t)bx * 32; e0 < j.count; e0 += (int64_t)nbx * 32) {
            const int64_t e = e0 + el;
            float acc = 0.f;
            if (e < j.count) {
                // 8 independent partial sums keep 8 strided loads in flight per thread (a single chain is latency bound:
                // nsrc/8 dependent L2 round trips); the combination order is fixed, so the result stays deterministic
                const float* p = scratch + j.src_off + e;
                float a8[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) a8[u] = 0.f;
                int k = sl;
                for (; k + 56 < j.nsrc; k += 64) {
#pragma unroll
                    for (int u = 0; u < 8; ++u) a8[u] += p[(int64_t)(k + 8 * u) * j.src_stride];
                }
                for (int u = 0; k < j.nsrc; k += 8, ++u) a8[u] += p[(int64_t)k * j.src_stride];
                acc = ((a8[0] + a8[1]) + (a8[2] + a8[3])) + ((a8[4] + a8[5]) + (a8[6] + a8[7]));
            }
            __syncthreads();
            red[sl][el] = acc;
            __syncthreads();
            if (sl == 0 && e < j.count) {
                float t = 0.f;
#pragma unroll
                for (int k = 0; k < 8; ++k) t += red[k][el];
                grad[j.dst_off + e] = t;
            }
        }
        return;
    }
    // few partial rows, many elements (split-K weight slabs): 16-byte accesses when every address is 16-byte aligned
    if (((j.src_off | j.src_stride | j.dst_off | j.count) & 3) == 0) {
        const int64_t n4 = j.count >> 2;
        for (int64_t e = (int64_t)bx * 256 + threadIdx.x; e < n4; e += (int64_t)nbx * 256) {
            const f32x4* p = reinterpret_cast<const f32x4*>(scratch + j.src_off) + e;
            const int64_t st4 = j.src_stride >> 2;
            f32x4 acc = p[0];
            // eight slab loads in flight, added in slab order (the plain loop was a chain of nsrc dependent L2 / HBM round
            // trips: 23 us per launch at 1280 samples, where the slabs hold 2 MB)
            int k = 1;
            for (; k + 8 <= j.nsrc; k += 8) {
                f32x4 v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = p[(int64_t)(k + u) * st4];
#pragma unroll
                for (int u = 0; u < 8; ++u) { acc[0] += v[u][0]; acc[1] += v[u][1]; acc[2] += v[u][2]; acc[3] += v[u][3]; }
            }
            for (; k < j.nsrc; ++k) {
                const f32x4 v = p[(int64_t)k * st4];
                acc[0] += v[0]; acc[1] += v[1]; acc[2] += v[2]; acc[3] += v[3];
            }
            reinterpret_cast<f32x4*>(grad + j.dst_off)[e] = acc;
        }
        return;
    }
    for (int64_t e = (int64_t)bx * 256 + threadIdx.x; e < j.count; e += (int64_t)nbx * 256) {
        const float* p = scratch + j.src_off + e;
        float acc = 0.f;
        for (int k = 0; k < j.nsrc; ++k) acc += p[(int64_t)k * j.src_stride];
        grad[j.dst_off + e] = acc;
    }
}
__global__ void __launch_bounds__(256) k_reduce_grads(ReduceJobs jobs, const float* scratch, float* grad) {
    __shared__ float red[8][32];
    (void)jobs;
    const ReduceJob j = kernarg_job<ReduceJob>((int)blockIdx.y);
    reduce_job_body(j, scratch, grad, (int)blockIdx.x, (int)gridDim.x, red, jobs.alt);
}
static int reduce_job_blocks(const ReduceJobs& jobs);
static inline int reduce_job_blocks_fwd(const ReduceJobs& jobs) { return reduce_job_blocks(jobs); }
hipError_t launch_reduce_grads(const ReduceJobs& jobs, const float* scratch, float* flat_grad, hipStream_t st) {
    if (jobs.n <= 0) return hipSuccess;
    // grid-stride loops inside; the result of every element is formed by one thread / one block in a fixed order whatever the grid.
    // Blocks per job: enough float4 lanes for the largest slab job, 64 ... 512 (the zero fill and the many-row jobs stride)
    hipLaunchKernelGGL(k_reduce_grads, dim3(reduce_job_blocks_fwd(jobs), jobs.n), dim3(256), 0, st, jobs, scratch, flat_grad);
    return hipGetLastError();
}

// Partial tiles of the batched weight-gradient launch (wgrad_batch.h) -> flat gradient.  Block (x, y): rows [16 x, 16 x + 16) of output
// tile y = (problem, lane slot); the partition is re-derived from the same struct the GEMM kernel used; partials are added in row
// order of the lane space (row-split tensors: first part, then the next) -- a fixed order.
__device__ __forceinline__ void reduce_wgrad_tile_body(const WgradBatchArgs& a, float* grad, int bxi, int byi) {
    const int p = byi >> 4, slot = byi & 15;
    const WgradLaneProblem& pr = a.prob[p];
    if ((pr.split_k && slot >= 8) || (pr.mode == 1 && slot >= 4)) return;
    const int half = pr.mode == 1 ? 0 : slot >> 3;
    const int cblk = pr.mode == 1 ? (slot & 1) : (slot & 3), sblk = pr.mode == 1 ? ((slot >> 1) & 1) : pr.sblk0[half] + ((slot & 7) >> 2);
    const int reps = pr.mode == 1 ? 4 : (pr.split_k ? 2 : 1), rep_stride = pr.mode == 1 ? 4 : 8;
    int start = 0;
    for (int i = 0; i < p; ++i) start += a.prob[i].len;
    const int end = start + pr.len;
    const int l0 = start / a.q, l1 = (end - 1) / a.q;
    const int64_t dst0 = pr.dst_off[half] + (int64_t)(cblk * 256) * pr.ld[half] + (int64_t)sblk * 256;
    const int ld = pr.ld[half];
    f32x4 acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    bool first = true;
    const int nterm = a.nterm > 1 ? a.nterm : 1;
    for (int tm = 0; tm < nterm; ++tm)
    for (int rep = 0; rep < reps; ++rep) {
        const int sl = slot + rep_stride * rep;
        for (int l = l0; l <= l1; ++l) {
            // ordinal of this problem's segment among the segments of lane l
            const int lo = l * a.q, hi = lo + a.q;
            int ord = 0, st2 = 0;
            for (int i = 0; i < p; ++i) {
                const int e2 = st2 + a.prob[i].len;
                if ((lo > st2 ? lo : st2) < (hi < e2 ? hi : e2)) ++ord;
                st2 = e2;
            }
            const f32x4* src = reinterpret_cast<const f32x4*>(a.partials + (int64_t)tm * a.term_stride + ((int64_t)(wgb_block(l, sl) * WGB_MAX_SEG + ord) << 16)) + bxi * 1024 + threadIdx.x;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const f32x4 v = src[i * 256];
                if (first) acc[i] = v;
                else { acc[i][0] += v[0]; acc[i][1] += v[1]; acc[i][2] += v[2]; acc[i][3] += v[3]; }
            }
            first = false;
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int idx4 = bxi * 1024 + i * 256 + threadIdx.x;       // float4 index inside the 256 x 256 tile
        const int row = idx4 >> 6, col = (idx4 & 63) << 2;
        float* d = grad + dst0 + (int64_t)row * ld + col;
        if (((dst0 | ld) & 3) == 0) *reinterpret_cast<f32x4*>(d) = acc[i];
        else { d[0] = acc[i][0]; d[1] = acc[i][1]; d[2] = acc[i][2]; d[3] = acc[i][3]; }
    }
}
__global__ void __launch_bounds__(256) k_reduce_wgrad_tiles(WgradBatchArgs a, float* grad) {
    reduce_wgrad_tile_body(a, grad, (int)blockIdx.x, (int)blockIdx.y);
}
// Both reductions behind a lane launch as ONE launch: blocks [0, 16 * 16 nprob) add partial tiles, the rest run the small jobs
// (GroupNorm / bias partials, split-K slabs of the 63-wide layers, zero fill) -- same bodies, same sums, one kernel boundary less.
struct ReduceAllArgs {
    ReduceJobs jobs;          // (first member: jobs are fetched through the kernel-argument segment)
    WgradBatchArgs wb;
    int job_blocks;           // blocks per job
};
__global__ void __launch_bounds__(256) k_reduce_all(ReduceAllArgs a, const float* scratch, float* grad) {
    __shared__ float red[8][32];
    const int n_tile_blocks = 16 * 16 * a.wb.nprob;
    const int b = blockIdx.x;
    if (b < n_tile_blocks) {
        reduce_wgrad_tile_body(a.wb, grad, b & 15, b >> 4);
        return;
    }
    const int jb = b - n_tile_blocks;
    const ReduceJob j = kernarg_job<ReduceJob>(jb / a.job_blocks);
    reduce_job_body(j, scratch, grad, jb % a.job_blocks, a.job_blocks, red, a.jobs.alt);
}
static int reduce_job_blocks(const ReduceJobs& jobs) {
    int64_t big = 0;
    for (int i = 0; i < jobs.n; ++i)
        if (jobs.job[i].nsrc > 0 && jobs.job[i].nsrc <= 64 && jobs.job[i].count > big) big = jobs.job[i].count;
    int gx = (int)((big / 4 + 255) / 256);
    return gx < 64 ? 64 : (gx > 512 ? 512 : gx);
}
hipError_t launch_reduce_all(const WgradBatchArgs& wb, const ReduceJobs& jobs, const float* scratch, float* flat_grad, hipStream_t st) {
    if (jobs.n <= 0) return launch_reduce_wgrad_tiles(wb, flat_grad, st);
    ReduceAllArgs a;
    a.jobs = jobs; a.wb = wb; a.job_blocks = reduce_job_blocks(jobs);
    hipLaunchKernelGGL(k_reduce_all, dim3((unsigned)(16 * 16 * wb.nprob + a.job_blocks * jobs.n)), dim3(256), 0, st, a, scratch, flat_grad);
    return hipGetLastError();
}
hipError_t launch_reduce_wgrad_tiles(const WgradBatchArgs& a, float* flat_grad, hipStream_t st) {
    hipLaunchKernelGGL(k_reduce_wgrad_tiles, dim3(16, (unsigned)(a.nprob * 16)), dim3(256), 0, st, a, flat_grad);
    return hipGetLastError();
}

__global__ void __launch_bounds__(256) k_sum_partials(const float* part, int n, float* out) {
    float acc = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) acc += part[i];
    const float tot = block_sum_256(acc);
    if (threadIdx.x == 0) out[0] = tot;
}
hipError_t launch_sum_partials(const float* part, int n, float* out, hipStream_t st) {
    hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(256), 0, st, part, n, out);
    return hipGetLastError();
}

__global__ void __launch_bounds__(256) k_sqnorm(const float* g, int64_t n, float* part) {
    float acc = 0.f;
    const int64_t n4 = n >> 2;
    const f32x4* g4 = reinterpret_cast<const f32x4*>(g);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        f32x4 v = g4[i];
        acc += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) { const float v = g[(n4 << 2) + threadIdx.x]; acc += v * v; }
    const float tot = block_sum_256(acc);
    if (threadIdx.x == 0) part[blockIdx.x] = tot;
}
hipError_t launch_sqnorm(const float* g, int64_t n, float* part, int* nblocks, hipStream_t st) {
    const int nb = grid_for(n / 4, 256, 1024);
    *nblocks = nb;
    hipLaunchKernelGGL(k_sqnorm, dim3(nb), dim3(256), 0, st, g, n, part);
    return hipGetLastError();
}

// Non-finite gradient guard: a NaN / Inf anywhere in the (all-reduced) gradient makes its squared norm non-finite; such a step
// is dropped on the device -- parameters, moments and EMA stay as they were -- and counted in sqnorm[1], which the host reads
// when it wants to (FusedAdam.nonfinite_steps()), not every step.
// (the counter update rides in the first thread of the optimizer kernel: one launch less in a step whose tail is latency-bound)
// 16-byte store of optimizer state.  wt != 0: WRITE-THROUGH (`sc0 sc1`): the line does not stay dirty in the XCD's L2.  Parameters,
// moments and EMA are not read again before the next step's optimizer launch, and ~130 MB of dirty lines at the end of the kernel are
// written back at the kernel boundary, in front of the next launch's first loads (the first kernel of the next step measured 17 us at
// any batch size with its waves parked on memory for 10 of them).  (asm: the string ends with s_nop 1 -- hipcc may reuse the data
// registers right behind the statement, cdna_hip_programming.md 5.7 item 1.)
__device__ __forceinline__ void store16(float* p, const f32x4& v, int wt) {
    if (wt) asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
    else *reinterpret_cast<f32x4*>(p) = v;
}
// one element of the update (losses.py:44-58 + torch.optim.Adam + ema.py:51); returns the new parameter value
__device__ __forceinline__ float adam_math(const AdamArgs& a, float coef, bool skip, float p, float g, float& m, float& v, float& s) {
    if (!skip) {
        g = g * coef;
        if (a.weight_decay != 0.f) g = g + a.weight_decay * p;   // torch.optim.Adam: grad = grad.add(param, alpha=weight_decay)
        p = adam_step(p, g, m, v, a.s);
    }
    s = s - a.ema_one_minus_decay * (s - p);                      // ema.py:51  s -= (1 - decay) * (s - p)
    return p;
}
__device__ __forceinline__ bool adam_skip(const AdamArgs& a, int64_t i) {
    return (i >= a.skip_lo[0] && i < a.skip_hi[0]) || (i >= a.skip_lo[1] && i < a.skip_hi[1]);
}
__device__ __forceinline__ float adam_elem(const AdamArgs& a, float coef, int64_t i) {
    const bool skip = adam_skip(a, i);
    float p = a.p[i], m = 0.f, v = 0.f, g = 0.f, s = 0.f;
    if (!skip) { g = a.g[i]; m = a.m[i]; v = a.v[i]; }
    if (a.ema) s = a.ema[i];
    p = adam_math(a, coef, skip, p, g, m, v, s);
    if (!skip) { a.m[i] = m; a.v[i] = v; a.p[i] = p; }
    if (a.ema) a.ema[i] = s;
    return p;
}
// squared gradient norm + clip coefficient shared by the two optimizer kernels; false: non-finite gradient, the step is dropped
__device__ __forceinline__ bool adam_prologue(const AdamArgs& a, float& coef) {
    // squared gradient norm: given (sqnorm[0]: the sharded step all-reduces it), or the per-block partials of k_sqnorm, which every
    // block adds up itself in k_sum_partials' order (n_part <= 1024 floats from L2: cheaper than the one-block launch it replaces)
    float sq;
    if (a.n_part > 0) {
        float acc = 0.f;
        for (int i = threadIdx.x; i < a.n_part; i += 256) acc += a.sq_part[i];
        sq = block_sum_256(acc);
        if (blockIdx.x == 0 && threadIdx.x == 0) a.sqnorm[0] = sq;
    } else {
        sq = a.sqnorm[0];
    }
    if (!isfinite(sq)) {
        if (blockIdx.x == 0 && threadIdx.x == 0) a.sqnorm[1] += 1.0f;
        return false;
    }
    // clip_grad_norm_ (losses.py:54-55): coef = max_norm / (total_norm + 1e-6), clamped to 1
    coef = a.grad_scale;
    if (a.grad_clip >= 0.f) {
        const float total_norm = sqrtf(sq) * a.grad_scale;
        float cc = a.grad_clip / (total_norm + 1e-6f);
        cc = cc > 1.0f ? 1.0f : cc;
        coef = a.grad_scale * cc;
    }
    return true;
}
__global__ void __launch_bounds__(256) k_adam_ema(AdamArgs a) {
    float coef;
    if (!adam_prologue(a, coef)) return;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * blockDim.x) adam_elem(a, coef, i);
}
hipError_t launch_adam_ema(const AdamArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(k_adam_ema, dim3(grid_for(a.n, 256, 4096)), dim3(256), 0, st, a);
    return hipGetLastError();
}

// ---- Adam + EMA + re-pack of the changed weights (kernels_api.h: AdamPackArgs) -----------------------------------------------------------
template <typename Job> __device__ __forceinline__ Job kernarg_job_at(size_t byte_off, int index) {
    static_assert(sizeof(Job) % 4 == 0, "jobs are copied as dwords");
    typedef const uint32_t __attribute__((address_space(4))) * ConstWords;
    ConstWords w = (ConstWords)__builtin_amdgcn_kernarg_segment_ptr() + byte_off / 4 + (size_t)index * (sizeof(Job) / 4);
    union { Job j; uint32_t u[sizeof(Job) / 4]; } c;
#pragma unroll
    for (unsigned i = 0; i < sizeof(Job) / 4; ++i) c.u[i] = w[i];
    return c.j;
}
// the part of one packed copy that a 64 x 64 tile of the source covers, from the updated values in LDS
template <typename T>
__device__ __forceinline__ void adam_pack_dst(const AdamPackDst& d, unsigned char* packed, const float (*tile)[65], int r0, int k0) {
    constexpr int EPL = FT<T>::EPL, KBS = FT<T>::KBS;
    constexpr int NKB = 64 / KBS, NCH = 2 * NKB * 64;            // FT blocks along the destination columns; 16-byte chunks of the tile's image
    T* base = reinterpret_cast<T*>(packed + d.off);
    const int drow0 = d.trans ? k0 : r0, dcol0 = d.koff + (d.trans ? r0 : k0);
    for (int c = threadIdx.x; c < NCH; c += 256) {
        const int lane = c & 63, blk = c >> 6;
        const int rb = blk / NKB, kb = blk % NKB;
        const int dr = rb * 32 + (lane & 31), dk = kb * KBS + (lane >> 5) * EPL;        // inside the tile's 64 x 64 image of the destination
        T vals[EPL];
#pragma unroll
        for (int e = 0; e < EPL; ++e) vals[e] = from_f32<T>(d.trans ? tile[dk + e][dr] : tile[dr][dk + e]);
        *reinterpret_cast<u32x4*>(base + FT<T>::index(drow0 + dr, dcol0 + dk, d.ktot)) = *reinterpret_cast<u32x4*>(vals);
    }
}
__global__ void __launch_bounds__(256) k_adam_pack(AdamPackArgs args) {
    __shared__ float tile[64][65];
    const AdamArgs& a = args.a;
    float coef;
    if (!adam_prologue(a, coef)) return;          // (dropped step: parameters and their packed copies stay as they are)
    const int b = blockIdx.x;
    if (b >= args.n_tiles) {
        // element ranges: biases (pairs feed the fp32 bias table), GroupNorm affine, dead parameters
        const int eb = b - args.n_tiles;
        int e = 0;
        for (int i = 1; i < args.n_elems; ++i)
            if (eb >= kernarg_job_at<AdamPackElems>(offsetof(AdamPackArgs, elems), i).block0) e = i;
        const AdamPackElems r = kernarg_job_at<AdamPackElems>(offsetof(AdamPackArgs, elems), e);
        const int nblk = (e + 1 < args.n_elems ? kernarg_job_at<AdamPackElems>(offsetof(AdamPackArgs, elems), e + 1).block0 : args.n_elem_blocks) - r.block0;
        if (r.off_b < 0 && ((r.off_a | r.len) & 3) == 0) {
            // plain range, 16-byte aligned (the dead pre_dense_cond range is 1.05 M floats): one float4 per thread and trip, loads of
            // the trip before its stores (a scalar loop here was a chain of dependent HBM round trips: 32 trips x ~2 us)
            const int n4 = r.len >> 2;
            for (int i = (eb - r.block0) * 256 + threadIdx.x; i < n4; i += nblk * 256) {
                const int64_t e0 = r.off_a + 4 * (int64_t)i;
                bool skip[4], any_live = false;
#pragma unroll
                for (int q = 0; q < 4; ++q) { skip[q] = adam_skip(a, e0 + q); any_live |= !skip[q]; }
                f32x4 P = *reinterpret_cast<const f32x4*>(a.p + e0), G = {0.f, 0.f, 0.f, 0.f}, M = G, V = G, S = G;
                if (any_live) { G = *reinterpret_cast<const f32x4*>(a.g + e0); M = *reinterpret_cast<const f32x4*>(a.m + e0); V = *reinterpret_cast<const f32x4*>(a.v + e0); }
                if (a.ema) S = *reinterpret_cast<const f32x4*>(a.ema + e0);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    float mq = M[q], vq = V[q], sq = S[q];
                    P[q] = adam_math(a, coef, skip[q], P[q], G[q], mq, vq, sq);
                    M[q] = mq; V[q] = vq; S[q] = sq;
                }
                if (any_live) {
                    store16(a.p + e0, P, args.write_through);
                    store16(a.m + e0, M, args.write_through);
                    store16(a.v + e0, V, args.write_through);
                }
                if (a.ema) store16(a.ema + e0, S, args.write_through);
            }
            return;
        }
        for (int i = (eb - r.block0) * 256 + threadIdx.x; i < r.len; i += nblk * 256) {
            const float pa = adam_elem(a, coef, r.off_a + i);
            if (r.off_b >= 0) {
                const float pb = adam_elem(a, coef, r.off_b + i);
                reinterpret_cast<float*>(args.packed)[r.cat_off + i] = pa + pb;
            }
        }
        return;
    }
    int t = 0;
    for (int i = 1; i < args.n_tensors; ++i)
        if (b >= kernarg_job_at<AdamPackTensor>(0, i).tile0) t = i;
    const AdamPackTensor T = kernarg_job_at<AdamPackTensor>(0, t);
    const int tiles_k = (T.K + 63) >> 6;
    const int tb = b - T.tile0;
    const int r0 = (tb / tiles_k) << 6, k0 = (tb % tiles_k) << 6;
    // 1. update the tile: thread (tr, tc) owns rows tr + 16 i, columns 4 tc .. 4 tc + 3; elements beyond the matrix are zeros in every copy.
    //    All loads of the thread's four rows are issued before the first store: behind a store hipcc cannot hoist the next row's loads
    //    (the five buffers may alias for all it knows) and the rows would be four dependent HBM round trips.
    const int tr = threadIdx.x >> 4, tc = threadIdx.x & 15;
    const bool vec = ((T.src_off | T.ld) & 3) == 0 && k0 + 64 <= T.K;
    if (vec) {
        f32x4 P[4], G[4], M[4], V[4], S[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = r0 + tr + 16 * i;
            const int64_t e0 = T.src_off + (int64_t)(r < T.R ? r : 0) * T.ld + k0 + 4 * tc;      // (rows beyond the matrix: loaded from row 0, never used)
            P[i] = *reinterpret_cast<const f32x4*>(a.p + e0); G[i] = *reinterpret_cast<const f32x4*>(a.g + e0);
            M[i] = *reinterpret_cast<const f32x4*>(a.m + e0); V[i] = *reinterpret_cast<const f32x4*>(a.v + e0);
            S[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (a.ema) S[i] = *reinterpret_cast<const f32x4*>(a.ema + e0);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = r0 + tr + 16 * i;
            float out[4] = {0.f, 0.f, 0.f, 0.f};
            if (r < T.R) {
                const int64_t e0 = T.src_off + (int64_t)r * T.ld + k0 + 4 * tc;
                bool any_live = false;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const bool skip = adam_skip(a, e0 + q);
                    any_live |= !skip;
                    float mq = M[i][q], vq = V[i][q], sq = S[i][q];
                    const float pq = adam_math(a, coef, skip, P[i][q], G[i][q], mq, vq, sq);
                    P[i][q] = pq; M[i][q] = mq; V[i][q] = vq; S[i][q] = sq;
                    out[q] = pq;
                }
                if (any_live) {
                    store16(a.p + e0, P[i], args.write_through);
                    store16(a.m + e0, M[i], args.write_through);
                    store16(a.v + e0, V[i], args.write_through);
                }
                if (a.ema) store16(a.ema + e0, S[i], args.write_through);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) tile[tr + 16 * i][4 * tc + q] = out[q];
        }
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = r0 + tr + 16 * i;
            float out[4] = {0.f, 0.f, 0.f, 0.f};
            if (r < T.R) {
                const int64_t e0 = T.src_off + (int64_t)r * T.ld + k0 + 4 * tc;
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (k0 + 4 * tc + q < T.K) out[q] = adam_elem(a, coef, e0 + q);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) tile[tr + 16 * i][4 * tc + q] = out[q];
        }
    }
    __syncthreads();
    // 2. the tile's part of every packed copy
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const AdamPackDst& dd = T.dst[d];
        if (dd.off < 0) continue;
        if (dd.f32) adam_pack_dst<float>(dd, args.packed, tile, r0, k0);
        else adam_pack_dst<__bf16>(dd, args.packed, tile, r0, k0);
    }
}
hipError_t launch_adam_pack(const AdamPackArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(k_adam_pack, dim3((unsigned)(a.n_tiles + a.n_elem_blocks)), dim3(256), 0, st, a);
    return hipGetLastError();
}


// ------------------------------------------------------------------------------------------------
// Runge-Kutta stage combination on the float64 ODE state (probability-flow ODE / likelihood):
//     out = [y +] scale * (c_0 K_0 + c_1 K_1 + ... )      left to right, no contraction (this file is built with
// -ffp-contract=off), i.e. the bits of the torch expression it replaces -- one launch instead of 2 n_terms + 1
// ------------------------------------------------------------------------------------------------
struct RkCombineArgs {
    const double* y;          // or null
    const double* k[8];
    double c[8];
    int n_terms;
    double scale;
    double* out;
    int64_t n;
};
__global__ void __launch_bounds__(256) k_rk_combine(RkCombineArgs a) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * blockDim.x) {
        double acc = a.k[0][i] * a.c[0];
#pragma unroll
        for (int j = 1; j < 8; ++j)
            if (j < a.n_terms) acc = acc + a.k[j][i] * a.c[j];
        acc = acc * a.scale;
        a.out[i] = a.y ? a.y[i] + acc : acc;
    }
}
extern "C" int dposer_rk_combine_f64(double* out, const double* y, const double* const* k_host, const double* coef_host, int32_t n_terms,
                                     double scale, int64_t n, void* stream) {
    DP_RANGE();
    DP_CHECK_ARG(out && k_host && coef_host && n_terms >= 1 && n_terms <= 8 && n >= 0, "bad argument");
    RkCombineArgs a;
    a.y = y; a.n_terms = n_terms; a.scale = scale; a.out = out; a.n = n;
    for (int j = 0; j < 8; ++j) { a.k[j] = j < n_terms ? k_host[j] : k_host[0]; a.c[j] = j < n_terms ? coef_host[j] : 0.0; }
    for (int j = 0; j < n_terms; ++j) DP_CHECK_ARG(k_host[j] != nullptr, "null stage pointer");
    if (n == 0) return DPOSER_OK;
    hipLaunchKernelGGL(k_rk_combine, dim3(grid_for(n, 256, 2048)), dim3(256), 0, (hipStream_t)stream, a);
    DP_CHECK_LAUNCH();
    return DPOSER_OK;
}

// ------------------------------------------------------------------------------------------------
// probability-flow ODE right-hand side around the score network (likelihood.py:60-65, 86-95; sampling.py:513-530):
//   drift(x, t) = -1/2 beta(t) x - 1/2 g(t)^2 score,  score = -model(x, 999 t) / std(t)          (sde_lib.py:100-104, utils.py:152-162)
// All samples of one evaluation share t.  `begin` prepares the network input from the float64 solver state and the upstream
// gradient of sum(drift * noise) w.r.t. the network output; `end` forms the drift and the Hutchinson estimate
// sum_i noise_i d(sum(drift * noise))/dx_i from the network's input gradient.  fp32 operation order = the torch expressions
// (and their autograd formulas) they replace; the per-sample sum runs over one wave instead of torch's reduction tree.
// ------------------------------------------------------------------------------------------------
struct PfRhsDev {
    SdeDev sde;
    float t;
    const double* state;      // begin: [B * D (+ B)]
    const float* noise;       // [B, D] or null
    float* x;                 // begin: out, end: in
    float* labels;            // begin: out [B]
    float* dout;              // begin: out [B, D] or null
    const float* out;         // end: network output [B, D]
    const float* dx;          // end: network input gradient [B, D] or null
    double* dstate;           // end: [B * D (+ B)]
    int64_t B;
    int D;
};
// VE SDE (round 6; sde_lib.py:258-268, utils.py:164-181, continuous): drift0 = 0, g = sigma(t) sqrt(2 ln(sigma_max / sigma_min)), the network is
// conditioned on sigma(t) and its output IS the score -- the same two kernels with the std division and the -1/2 beta x term gone.
__global__ void __launch_bounds__(256) k_pf_rhs_begin(PfRhsDev d) {
    const int64_t n = d.B * d.D;
    const bool ve = d.sde.kind == SDE_VE;
    const SdeAt at = sde_at(d.sde, d.t);                                      // (sub-VP / VP: the functions the call sites always used, in their order)
    const float g = ve ? at.g : sde_diffusion(d.sde, d.t);
    const float g2 = g * g;                                                  // diffusion[:, None] ** 2
    const float sd = ve ? 1.0f : sde_std(d.sde, sde_lmc(d.sde, d.t));
    const float label = ve ? at.label : d.t * 999.0f;                        // utils.py:152 / :173
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        d.x[i] = (float)d.state[i];
        if (i < d.B) d.labels[i] = label;
        if (d.dout) {
            // autograd of  drift0 - (g2 * score) * 0.5,  score = (-out) / std  (VE: score = out)  with upstream gradient `noise`
            const float gscore = ((-d.noise[i]) * 0.5f) * g2;
            d.dout[i] = ve ? gscore : -(gscore / sd);
        }
    }
}
__global__ void __launch_bounds__(256) k_pf_rhs_end(PfRhsDev d) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= d.B) return;
    const bool ve = d.sde.kind == SDE_VE;
    const float g = ve ? sde_at(d.sde, d.t).g : sde_diffusion(d.sde, d.t);
    const float g2 = g * g;
    const float sd = ve ? 1.0f : sde_std(d.sde, sde_lmc(d.sde, d.t));
    const float a = ve ? 0.0f : -0.5f * sde_beta(d.sde, d.t);                // -0.5 * beta_t (VE: drift0 = zeros_like(x), sde_lib.py:261)
    float acc = 0.f;
    for (int c = lane; c < d.D; c += 64) {
        const int64_t i = row * d.D + c;
        const float score = ve ? d.out[i] : (-d.out[i]) / sd;
        const float drift = a * d.x[i] - (g2 * score) * 0.5f;
        d.dstate[i] = (double)drift;
        if (d.dx) {
            const float nz = d.noise[i];
            const float vjp = d.dx[i] + nz * a;
            acc += vjp * nz;
        }
    }
    if (d.dx) {
        for (int s = 32; s >= 1; s >>= 1) acc += __shfl_xor(acc, s);
        if (lane == 0) d.dstate[d.B * d.D + row] = (double)acc;
    }
}
static SdeDev pf_sde_dev(const dposer_sde_desc* s) {
    SdeCfg c;
    c.kind = s->kind == DPOSER_SDE_VP ? SDE_VP : (s->kind == DPOSER_SDE_VE ? SDE_VE : SDE_SUBVP);
    c.beta_0 = s->beta_min; c.beta_1 = s->beta_max; c.N = s->N; c.T = (float)s->T;      // (VE: the beta fields carry sigma_min / sigma_max)
    return make_sde_dev(c);
}
extern "C" int dposer_pf_ode_rhs_begin(const dposer_sde_desc* sde, float t, const double* state, const float* noise, float* x, float* labels,
                                       float* dout, int64_t batch, int32_t dim, void* stream) {
    DP_RANGE();
    DP_CHECK_ARG(sde && state && x && labels && batch >= 0 && dim >= 1, "bad argument");
    DP_CHECK_ARG(sde->kind == DPOSER_SDE_VP || sde->kind == DPOSER_SDE_SUBVP || sde->kind == DPOSER_SDE_VE, "unknown SDE kind");
    DP_CHECK_ARG(!dout || noise, "dout needs noise");
    if (batch == 0) return DPOSER_OK;
    PfRhsDev d{};
    d.sde = pf_sde_dev(sde); d.t = t; d.state = state; d.noise = noise; d.x = x; d.labels = labels; d.dout = dout; d.B = batch; d.D = dim;
    hipLaunchKernelGGL(k_pf_rhs_begin, dim3(grid_for(batch * dim, 256, 2048)), dim3(256), 0, (hipStream_t)stream, d);
    DP_CHECK_LAUNCH();
    return DPOSER_OK;
}
extern "C" int dposer_pf_ode_rhs_end(const dposer_sde_desc* sde, float t, const float* x, const float* model_out, const float* dx,
                                     const float* noise, double* dstate, int64_t batch, int32_t dim, void* stream) {
    DP_RANGE();
    DP_CHECK_ARG(sde && x && model_out && dstate && batch >= 0 && dim >= 1, "bad argument");
    DP_CHECK_ARG(sde->kind == DPOSER_SDE_VP || sde->kind == DPOSER_SDE_SUBVP || sde->kind == DPOSER_SDE_VE, "unknown SDE kind");
    DP_CHECK_ARG(!dx || noise, "dx needs noise");
    DP_CHECK_ARG((batch + 3) / 4 < (int64_t)1 << 31, "batch too large");
    if (batch == 0) return DPOSER_OK;
    PfRhsDev d{};
    d.sde = pf_sde_dev(sde); d.t = t; d.x = const_cast<float*>(x); d.out = model_out; d.dx = dx; d.noise = noise; d.dstate = dstate;
    d.B = batch; d.D = dim;
    hipLaunchKernelGGL(k_pf_rhs_end, dim3((unsigned)((batch + 3) / 4)), dim3(256), 0, (hipStream_t)stream, d);
    DP_CHECK_LAUNCH();
    return DPOSER_OK;
}
