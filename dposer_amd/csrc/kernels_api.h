// Elementwise / layout / optimizer kernels of the score path (implemented in elementwise.hip).
#pragma once
#include "common.h"
#include "wgrad_batch.h"
#include "gemm_api.h"
#include "optim_dev.h"   // AdamScalars

// ---- weight packing -----------------------------------------------------------------------------
struct PackJob {
    int64_t dst_off;      // byte offset inside the packed workspace
    int64_t src_off;      // element offset inside the flat fp32 parameter buffer
    int ktot;             // columns of the destination FT matrix
    int koff;             // first destination column written by this job
    int rows_pad, kpad;   // extent written (multiples of 32 / KBS), zero-filled outside the source
    int rows_valid, cols_valid, ld;
    int trans;            // 0: dst[r][koff+k] = src[r*ld + k]     1: dst[r][koff+k] = src[k*ld + r]
    int f32;              // destination element type: 1 fp32, 0 bf16
    int split;            // bf16 destinations: 0 = bf16(v), 1 = high part bf16(v), 2 = low part bf16(v - float(bf16(v)))
};
constexpr int MAX_PACK_JOBS = 40;
struct PackJobs {
    PackJob job[MAX_PACK_JOBS];
    int n;
};
hipError_t launch_pack(const PackJobs& jobs, const float* flat, void* packed, hipStream_t st);
// dst[i] = flat[a_off[i/H] + i%H] + flat[b_off[..]]
struct BiasCatJobs {
    int64_t a_off[8], b_off[8];
    int n, H;
};
hipError_t launch_bias_cat(const BiasCatJobs& j, const float* flat, float* dst, hipStream_t st);

#include "sde_dev.h"   // SdeCfg, SdeDev

// ---- input preparation ---------------------------------------------------------------------------
struct PrepArgs {
    const float* x;        // [B][D] fp32 row-major
    const float* labels;   // [B] (per-sample t path) or null
    const float* freq;     // [E/2] positional frequencies, or fourier W
    void* xin;             // FT [Bpad][Dpad]
    void* emb;             // FT [Bpad][E] or null
    int64_t B, Bpad;
    int D, Dpad, E;
    int fourier;
    int f32;
};
hipError_t launch_prep_infer(const PrepArgs& a, hipStream_t st);

struct PrepTrainArgs {
    const float* x0;       // [B][D] clean (normalised) poses
    const float* t_in;     // [B] injected t or null (-> Philox STREAM_TRAIN_T)
    const float* z_in;     // [B][D] injected z or null (-> Philox STREAM_TRAIN_Z)
    const float* freq;
    void* xin;             // FT [Bpad][Dpad]  perturbed data
    void* emb;             // FT [Bpad][E]
    float* t_out;          // [Bpad]
    float* z_out;          // [Bpad][Dpad] fp32 row-major
    int64_t B, Bpad;
    int D, Dpad, E;
    int fourier, f32;
    SdeCfg sde;
    float eps;             // smallest t (1e-5)
    uint64_t seed;
    uint32_t step;
};
hipError_t launch_prep_train(const PrepTrainArgs& a, hipStream_t st);

// time embedding rows for a list of labels (labels == null: every row uses label0): emb FT32 [Npad][E]
hipError_t launch_time_embed(const float* labels, float label0, int64_t n, int64_t npad, const float* freq, int E, int fourier, float* emb_ft32, hipStream_t st);
// VE labels in place: t[i] -> sigma(t[i]) = sigma_min * (sigma_max / sigma_min)^t with the DEVICE's powf -- the value every kernel that perturbs with /
// divides by sigma(t) forms for itself (host libm's powf may differ by an ulp)
hipError_t launch_ve_labels(float* t_inout, int n, float smin, float ratio, hipStream_t st);

// ---- output stages ---------------------------------------------------------------------------------
struct OutModelArgs {      // ScoreModelFC.forward tail: res / used_sigmas   (model.py:189-196)
    const float* res;      // [Bpad][Cp]
    const float* labels;   // [B]
    const float* sigmas;   // [num_scales]
    float* out;            // [B][D]
    int64_t B;
    int D, Cp, num_scales;
    int scale_by_sigma, fourier;
};
hipError_t launch_out_model(const OutModelArgs& a, hipStream_t st);

// What the four update kernels of the samplers share (scorefc.hip: update_common fills it from the handle, the workspace and the call).
// t and step sit with the pointers, no padding anywhere: the blocks keep their sizes, and each kernel's first batch of scalar loads
// touches every cache line of its argument block (with t behind `seed` k_langevin_norms took 0.6 us longer per launch).
struct UpdateCommon {
    const float* res;      // [Bpad][Cp] post_dense output at x
    float* x;              // [B][D] state, updated in place
    float* x_mean;         // [B][D]
    void* xin;             // FT [Bpad][Dpad]: the new state as the next network input
    const float* sigmas;
    float t;               // the launch's shared time
    uint32_t step;
    int64_t B, Bpad;
    int D, Dpad, Cp, num_scales;
    int f32;
    int scale_by_sigma;
    SdeCfg sde;
    uint64_t seed;
};
struct EmUpdateArgs : UpdateCommon {   // EulerMaruyamaPredictor.update_fn + imputation (sampling.py:182-188, 416-420)
    // res == null: no predictor step, only impute A + pack
    const float* obs;      // completion: observation [B][D] or null
    const float* mask;     // completion: mask [B][D]
    float* traj;           // [B][D] slot for this step or null
    float* x_ft;           // optional: the new state again as fp32 FT [Bpad][Dpad] (start of the fused sampler fast path)
    const float* z_pred;   // injected predictor noise [B][D] or null (-> Philox); not read under probability flow
    const float* z_impB;   // injected imputation noise after the predictor, or null
    const float* z_impA;   // injected imputation noise before the NEXT predictor step, or null
    float t_next;          // next timestep (< 0: last step, no look-ahead imputation)
    int pf;                // probability-flow ODE step: drift factor 0.5, no diffusion, no predictor draw (sde_lib.py:102-104)
};
hipError_t launch_em_update(const EmUpdateArgs& a, hipStream_t st);
// fp32 FT [Bpad][Dpad] -> row-major [B][D] (end of the fused sampler fast path); any of the two pairs may be null
hipError_t launch_ft_to_rows(const float* a_ft, float* a, const float* b_ft, float* b, int64_t B, int64_t Bpad, int D, int Dpad, hipStream_t st);

// What the prior and loop kernels that read the network output at one shared t have in common (scorefc.hip: score_out fills it from the call
// context).  UpdateCommon's care: the pointers first, t with them, no padding hole, and the size a multiple of 8, so that the derived
// blocks start their own pointers right behind it and a kernel's first batch of scalar loads covers the block from its start.
struct ScoreOut {
    const float* res;      // [Bpad][Cp] post_dense output at x_t
    const float* sigmas;
    float t;               // the launch's shared time
    int scale_by_sigma;
    int64_t B;
    int D, Dpad, Cp, num_scales;
    SdeCfg sde;
};
static_assert(sizeof(ScoreOut) == 2 * 8 + 2 * 4 + 8 + 4 * 4 + sizeof(SdeCfg), "ScoreOut has a padding hole");
struct DenoiseArgs : ScoreOut {   // one_step_denoise + prior loss (run/completion.py:105-149, run/smplify.py:69-107)
    const float* x0;       // [B][D]
    const float* xt;       // [B][Dpad] perturbed data (fp32 row-major)
    float* x0_hat;         // [B][D] or null
    float* grad;           // [B][D] d loss / d x0 (analytic, x0_hat detached) or null
    float* loss_part;      // per-block partial sums
    float inv_n;           // 1/n of the reduction (mean: 1/(B*D), sum/batch: 1/B)
    int weighted;
};
hipError_t launch_denoise(const DenoiseArgs& a, int* nblocks, hipStream_t st);

struct PerturbSharedArgs { // x_t = mean + std*z at one shared t; writes xin (FT) and xt (fp32)
    const float* x0;
    const float* z_in;     // injected or null (-> Philox STREAM_PRIOR)
    void* xin;
    float* xt;             // [Bpad][Dpad]
    float t;
    int64_t B, Bpad;
    int D, Dpad, f32;
    SdeCfg sde;
    uint64_t seed;
    uint32_t step;
};
hipError_t launch_perturb_shared(const PerturbSharedArgs& a, hipStream_t st);

struct DdimStepArgs : ScoreOut {   // one step of multi_step_denoise behind its network evaluation (run/completion.py:112-129); the last step also forms the loss
    // t: time_traj[i]
    float* xt;             // [Bpad][Dpad] current state (fp32 row-major), updated in place
    void* xin;             // FT [Bpad][Dpad]: the next evaluation's network input
    const float* x0;       // last step: [B][D] clean poses
    float* x0_hat;         // last step: [B][D] the multi-step estimate, or null
    float* grad;           // last step: [B][D] d loss / d x0 (the estimate is detached) or null
    float* loss_part;      // last step: per-block partial sums
    int64_t Bpad;
    float t_next;          // time_traj[i + 1]
    float t0;              // time_traj[0]: the SNR of the loss weight (completion.py:127-128)
    float inv_n;
    int weighted;
    int last;              // 1: no state is written back; x0_hat / grad / loss_part are
    int f32;
};
hipError_t launch_ddim_step(const DdimStepArgs& a, int* nblocks, hipStream_t st);

struct DpmUpdateArgs : UpdateCommon {   // one DPM-Solver++ (multistep, data prediction) step behind its network evaluation at t = s_i (dposer_dpm_sampler)
    // x: read and written as [B][D] rows; x_mean: unused (null)
    float* hist;           // [B][D] data prediction of the previous step: read when use_hist, always overwritten with this step's (null: neither)
    float* x0_hat;         // last step: [B][D] this step's data prediction, else null
    const float* obs;      // completion: observation [B][D] or null
    const float* mask;     // completion: mask [B][D]
    float* traj;           // [B][D] slot of this step (the state before the look-ahead imputation) or null
    const float* z_imp;    // injected draw of the imputation at t_next, or null (-> Philox STREAM_IMPUTE_A at step + 1)
    float t_next;          // s_{i+1} when the state is imputed there (completion, not the last step); < 0: no imputation
    float cx, c0, c1;      // x <- cx x + c0 D_i + c1 D_{i-1}: the host's float64 schedule rounded once (dposer_dpm_coefficients)
    int use_hist;          // effective order 2: c1 D_{i-1} is read and added
};
hipError_t launch_dpm_update(const DpmUpdateArgs& a, hipStream_t st);

struct RedDiffArgs : ScoreOut {   // MotionDenoise.RED_Diff behind its network evaluation (run/motion_denoising.py:145-154)
    const float* x0;       // [B][D]
    const float* z_in;     // the perturbation's injected z, or null (-> the same Philox STREAM_PRIOR draws as k_perturb_shared)
    float* eps_pred;       // [B][D] noise prediction -score * std, or null
    float* grad;           // [B][D] weight (eps_pred - z) inv_batch, or null
    float* loss_part;      // per-block partial sums
    uint64_t seed;
    float inv_batch;
    uint32_t step;
};
hipError_t launch_red_diff(const RedDiffArgs& a, int* nblocks, hipStream_t st);

struct CompletionUpdateArgs : ScoreOut {   // one optimisation step of DPoserComp.optimize (run/completion.py:167-207) after the network evaluation
    const float* xt;       // [Bpad][Dpad] perturbed data
    const float* obs;      // [B][D]
    const float* mask;     // [B][D]
    float* x;              // [B][D] optimisation variable, updated in place
    float* m;              // [B][D] Adam first moment
    float* v;              // [B][D] Adam second moment
    float inv_n;           // 1 / (B * D): both losses are means over the batch (completion.py:147, nn.MSELoss)
    float w_prior, w_data; // loss weights of this step (completion.py:151-155)
    int weighted;
    AdamScalars s;         // torch.optim.Adam scalars of this step
};
hipError_t launch_completion_update(const CompletionUpdateArgs& a, hipStream_t st);

struct LangevinArgs : UpdateCommon {   // LangevinCorrector.update_fn (sampling.py:282-302) around one network evaluation at a shared t
    // x_mean: out (update phase); xin: written by the update phase, or null
    const float* noise;    // injected noise [B][D] or null (-> Philox STREAM_LANGEVIN)
    float* part;           // norms phase: per-block partial sums, [2][nblocks]
    const float* norm_sums;// update phase: [2] = sum_b ||grad_b||, sum_b ||noise_b|| over the GLOBAL batch
    float alpha, snr, inv_global_batch;
};
hipError_t launch_langevin_norms(const LangevinArgs& a, int* nblocks, hipStream_t st);
hipError_t launch_sum_partials2(const float* part, int n, float* out2, hipStream_t st);   // out2[k] = sum part[k*n .. k*n+n)
hipError_t launch_langevin_update(const LangevinArgs& a, hipStream_t st);
hipError_t launch_pack_rows(const float* x, void* xin, int64_t B, int64_t Bpad, int D, int Dpad, int f32, hipStream_t st);

// ---- one-call predictor-corrector sampler: the predictors that are not Euler-Maruyama, and annealed Langevin dynamics ----
struct PcPredArgs : UpdateCommon {     // ReverseDiffusion / AncestralSampling / None predictor + imputation (sampling.py:210-270, 416-420)
    // res: not read by the 'none' predictor
    const float* obs;      // completion: observation [B][D] or null
    const float* mask;
    float* traj;           // [B][D] slot of this step or null
    const float* z_pred;   // injected predictor noise or null (-> Philox STREAM_EM_NOISE); not read under pf / by 'none'
    const float* z_impB;   // injected imputation noise after the predictor, or null
    const float* z_impA;   // injected imputation noise ahead of the NEXT step (corrector 'none' only), or null
    float t_next;          // < 0: no look-ahead imputation
    PcTab tab;             // this step's table entries, by value
    int pred;              // DPOSER_PC_PRED_REVERSE_DIFFUSION / _ANCESTRAL / _NONE
    int pf;
};
hipError_t launch_pc_pred_update(const PcPredArgs& a, hipStream_t st);
struct AldArgs : UpdateCommon {        // AnnealedLangevinDynamics.update_fn (sampling.py:319-339), one inner step at a shared t
    // x_mean: out, or null: not stored (a predictor update that follows overwrites it)
    const float* obs;      // last inner step of a completion: imputation after the corrector (sampling.py:416-420), else null
    const float* mask;
    const float* noise;    // injected noise [B][D] or null (-> Philox STREAM_LANGEVIN at `step`)
    const float* z_imp;    // the imputation's injected draw or null (-> Philox STREAM_IMPUTE_A at `imp_step`)
    float alpha, snr;
    uint32_t imp_step;
};
hipError_t launch_ald_update(const AldArgs& a, hipStream_t st);

// ---- one-call MCG / DPS guided sampler (sampling.py:191-207 around sde_lib.py:98-109): two passes around the batch-wide norm and the dgrad ----
struct GuidedArgs : UpdateCommon {
    // res: post_dense output at x, kept with the activations; x_mean: out = y_mean (the mean does not carry the guidance)
    const float* obs;      // observation [B][D]
    const float* mask;     // mask [B][D]
    float* traj;           // [B][D] slot of this step or null
    const float* z_pred;   // injected predictor noise [B][D] or null (-> Philox STREAM_EM_NOISE at `step`)
    const float* z_imp;    // MCG: injected imputation noise or null (-> Philox STREAM_IMPUTE_B at `step`)
    void* dres;            // resid pass: FT [Bpad][Cp], d norm / d res TIMES norm (the backward is linear: the update pass divides)
    float* part;           // resid pass: per-block partial sums of r^2
    const float* norm_sq;  // update pass: [1] = sum of the partials
    const float* dx;       // update pass: [B][D] = J_res^T dres
    int32_t* nonfinite;    // update pass: atomicMin of `step` where an element of the gradient is not finite
    float grad_step;
    int project;           // 1: MCG's imputation behind the step
};
hipError_t launch_guided_resid(const GuidedArgs& a, int* nblocks, hipStream_t st);
hipError_t launch_guided_update(const GuidedArgs& a, hipStream_t st);

// ---- one-call DPS sampler on observed 3D joints: the passes around the joint-residual stage (jointguide.hip) and the dgrad ----
struct JointGuidedArgs : UpdateCommon {
    // res: post_dense output at x, kept with the activations; x_mean: out = y_mean
    float* y0;             // y0 pass: [B][D] Tweedie estimate, the stage's input
    const float* v;        // dres / update pass: [B][D] the stage's 1/2 d s / d y0
    const float* s;        // update pass: [B] the stage's sums (norm_scope 1: norm_b = sqrt(s[b]))
    const float* norm_sq;  // update pass, norm_scope 0: [1] = sum_b s[b]
    void* dres;            // dres pass: FT [Bpad][Cp], d norm / d res TIMES norm
    const float* dx;       // update pass: [B][D] = J_res^T dres
    float* traj;           // [B][D] slot of this step or null
    const float* z_pred;   // injected predictor noise [B][D] or null (-> Philox STREAM_EM_NOISE at `step`)
    int32_t* nonfinite;    // update pass: atomicMin of `step` where an element of the gradient is not finite
    float grad_step;
    int norm_scope;        // 0: one norm over the batch, 1: one per row
};
hipError_t launch_joint_guided_y0(const JointGuidedArgs& a, hipStream_t st);
hipError_t launch_joint_guided_dres(const JointGuidedArgs& a, hipStream_t st);
hipError_t launch_joint_guided_update(const JointGuidedArgs& a, hipStream_t st);

struct DsmArgs {           // get_sde_loss_fn tail (losses.py:121-131) + d loss / d res
    const float* res;      // [Bpad][Cp]
    const float* t;        // [Bpad]
    const float* z;        // [Bpad][Dpad]
    const float* sigmas;
    void* dres;            // FT [Bpad][Cp]
    float* loss_part;      // per-block partial sums of the (already normalised) loss
    float* cs_part;        // optional [blocks][Cp]: per-block column sums of dres (post_dense bias gradient partials)
    int64_t B, Bpad;
    int D, Dpad, Cp, num_scales, scale_by_sigma, f32, fourier;
    float grad_scale;      // 1/(B*D) for reduce_mean
    SdeCfg sde;
};
hipError_t launch_dsm(const DsmArgs& a, int* nblocks, hipStream_t st);

struct SiLUBwdReduceArgs {  // dU = (sum over the k-splits of the time-branch dgrad) * act'(u); column sums of the stored dU per block
    const float* part;     // [nsplit][Spad][N] fp32 FT (EpiPartialFT)
    int nsplit;
    int64_t split_stride;
    const void* pre;       // u, FT [Spad][N]
    void* out;             // dU, FT [Spad][N]
    float* cs_part;        // [blocks][N]
    int N, act, f32;
    int64_t B, Spad;
};
hipError_t launch_silu_bwd_reduce(const SiLUBwdReduceArgs& a, int max_blocks, int* nblocks, hipStream_t st);
// the same reduction walked in FRAGMENT-TILE order (fp32 storage; bf16x3 mode at every batch size): every access is a coalesced 1-KiB run
// (the row-major walk above touches one 16-byte chunk per 1-KiB block); optionally writes dU's bf16 operand planes too.  Column sums:
// one partial row per row-block group (`*nblocks` rows of N floats in cs_part).
hipError_t launch_silu_bwd_reduce_ft(const SiLUBwdReduceArgs& a, void* out_hi, void* out_lo, int max_blocks, int* nblocks, hipStream_t st);

struct DresArgs {          // d res = d out / used_sigmas  (backward of model.py:192-194), FT store
    const float* dout;     // [B][D]
    const float* labels;   // [B]
    const float* sigmas;
    void* dres;            // FT [Bpad][Cp]
    int64_t B, Bpad;
    int D, Cp, num_scales, scale_by_sigma, fourier, f32;
};
hipError_t launch_dres_from_dout(const DresArgs& a, hipStream_t st);

// ---- layout helpers ---------------------------------------------------------------------------------
// out FT [Cpad][Spad] = transpose of in FT [Spad][C]
hipError_t launch_ft_transpose(int f32, const void* in, void* out, int64_t Spad, int C, hipStream_t st);
// fp32 FT [rows_pad][K] -> bf16 FT planes hi = bf16(x), lo = bf16(x - hi) of the same shape (bf16 x 3 precision mode)
hipError_t launch_split_ft32(const void* src, void* hi, void* lo, int64_t rows_pad, int K, hipStream_t st);
// part[chunk][c] = sum over the chunk's samples of in[s][c];  returns number of chunks.  `rider` (optional): a list of partials summed
// into out[0] by one extra block of the same launch (the DSM loss of the step: k_sum_partials' summation order, no launch of its own)
struct SumJob {
    const float* part;
    int n;
    float* out;
};
hipError_t launch_colsum(int f32, const void* in, float* part, int64_t Spad, int C, int* nchunks, hipStream_t st, const SumJob* rider = nullptr);

// ---- gradient finalisation and optimizer --------------------------------------------------------------
struct ReduceJob {
    int64_t dst_off;       // element offset in the flat gradient
    int64_t count;
    int64_t src_off;       // element offset in the scratch buffer
    int64_t src_stride;
    int nsrc;              // 0: fill [dst_off, dst_off + count) with zeros (parameters that never get a gradient);
                           // -1: ReduceJobs::alt[0] = sum of scratch[src_off .. src_off + count) in k_sum_partials' order (the step's loss)
};
constexpr int MAX_REDUCE_JOBS = 48;
struct ReduceJobs {
    ReduceJob job[MAX_REDUCE_JOBS];
    int n;
    float* alt;            // destination of the nsrc = -1 job (outside the flat gradient)
};
hipError_t launch_reduce_grads(const ReduceJobs& jobs, const float* scratch, float* flat_grad, hipStream_t st);
hipError_t launch_reduce_wgrad_tiles(const WgradBatchArgs& a, float* flat_grad, hipStream_t st);   // wgrad_batch.h: partial tiles -> flat gradient
// both of the above in one launch (the partial tiles of a lane launch + the small jobs behind it)
hipError_t launch_reduce_all(const WgradBatchArgs& a, const ReduceJobs& jobs, const float* scratch, float* flat_grad, hipStream_t st);
hipError_t launch_sum_partials(const float* part, int n, float* out, hipStream_t st);             // out[0] = sum(part[0..n))
hipError_t launch_sqnorm(const float* g, int64_t n, float* part, int* nblocks, hipStream_t st);   // partial sums of g^2

struct AdamArgs {          // losses.py:44-58 optimize_fn + torch.optim.Adam + ema.py:32-51, one pass
    float* p;
    const float* g;
    float* m;
    float* v;
    float* ema;            // may be null
    int64_t n;
    int64_t skip_lo[2], skip_hi[2];   // parameter ranges without gradient (Adam skipped, EMA still applied)
    float* sqnorm;         // device scalars: [0] sum of g^2 over the whole flat gradient (before grad_scale), [1] dropped-step counter
    const float* sq_part;  // n_part > 0: per-block partials of k_sqnorm, summed by the kernel itself (and published in sqnorm[0])
    int n_part;
    float grad_scale;      // applied to g before anything else (1/world_size)
    float grad_clip;       // < 0: disabled
    AdamScalars s;         // step_size = lr / (1 - beta1^t), bc2_sqrt = sqrt(1 - beta2^t)
    float ema_one_minus_decay;
    float weight_decay;    // torch.optim.Adam(weight_decay): grad += weight_decay * param (after the clip, before the moments); 0 = off
};
hipError_t launch_adam_ema(const AdamArgs& a, hipStream_t st);

// ---- the same update fused with the re-packing of the weights it changes (one pass over the optimizer state) --------------------
// A weight matrix W [R][K] (row-major, leading dimension ld) of the flat buffer and the packed copies the GEMMs read: every 64 x 64
// tile of W is updated by one block, which then writes the tile's part of each copy from LDS -- instead of k_adam_ema writing the
// parameters and k_pack / k_bias_cat of the NEXT step reading them back (33 MB read twice or three times, 2 launches).
struct AdamPackDst {
    int64_t off;          // byte offset in the packed workspace; < 0: unused
    int ktot, koff;       // destination FT matrix has ktot columns, this tensor starts at column koff
    int trans;            // 1: destination rows = columns of W (dgrad copies)
    int f32;              // destination element type
};
struct AdamPackTensor {
    int64_t src_off;      // element offset of W in the flat buffers
    int R, K, ld;
    int tile0;            // index of the tensor's first tile among all tiles of the launch
    AdamPackDst dst[3];
};
struct AdamPackElems {    // a range that is not a packed matrix (biases, GroupNorm affine, dead parameters, ...)
    int64_t off_a, off_b; // off_b >= 0: a second range of the same length updated by the same thread (dense bias | dense_t bias) ...
    int64_t cat_off;      // ... whose sums a[i] + b[i] go to the fp32 bias table at this float offset of the packed workspace
    int len;
    int block0;           // index of the range's first block among the element blocks
};
constexpr int ADAMPACK_MAX_TENSORS = 16, ADAMPACK_MAX_ELEMS = 28;
struct AdamPackArgs {
    AdamPackTensor tensor[ADAMPACK_MAX_TENSORS];      // (first member: fetched through the kernel-argument segment)
    AdamPackElems elems[ADAMPACK_MAX_ELEMS];
    int n_tensors, n_elems, n_tiles, n_elem_blocks;
    AdamArgs a;
    unsigned char* packed;
    int64_t bias_cat_off; // byte offset of the bias table in `packed`
    int write_through;    // 1: parameters / moments / EMA leave as write-through stores (no dirty L2 lines behind the launch)
};
hipError_t launch_adam_pack(const AdamPackArgs& a, hipStream_t st);

// ---- body-model internals that jointguide.hip shares with fk.hip (implemented there) ----------------------------------------------------
int body_num_joints(dposer_body_t h);                                 // 0 for a null handle
// the reverse walk of dposer_fk_joints_backward alone, on the transforms A [B][n_out][12] of a dposer_fk_joints(rel_transforms = A) call over
// the same segments; arguments as in that entry, already checked
int fk_joints_backward_launch(dposer_body_t h, const float* const* pose_segments_host, const int32_t* segment_joints_host, int32_t num_segments,
                              const float* j_rest, int32_t j_rest_batched, const float* A, const float* d_joints, int64_t d_joints_ld, int32_t n_out,
                              float* const* d_pose_segments_host, float* d_jrest, int64_t batch, hipStream_t st);
