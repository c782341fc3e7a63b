/*
 * dposer_hip.h -- C ABI of libdposer_hip.so: the MI355X (gfx950) implementation of DPoser's
 * diffusion hot path.
 *
 * The reference (moonbow721/DPoser) has NO native boundary: the path sits behind Python call
 * sites.  Each entry point below therefore names the reference *Python*
 * function it replaces (paths relative to the reference root); dposer_amd/ binds them with
 * ctypes (dposer_amd/_C.py) and INTEGRATION.md shows the binding a reference maintainer adds.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless its name ends in _host;
 *   - matrices are fp32 row-major exactly as the reference's torch tensors ([B, D] poses, ...);
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream);
 *     kernels are only enqueued, never synchronised, no allocation happens inside a call;
 *   - scratch memory is caller-owned: query *_bytes(), allocate once (e.g. a torch uint8
 *     tensor), pass the pointer;
 *   - return value: 0 = ok, <0 = error (DPOSER_ERR_*), message via dposer_last_error().  The entries that evaluate the network at one
 *     time shared by the batch (the samplers, dposer_langevin_step, the dposer_prior_* family, dposer_completion_optimize) check every
 *     argument before anything else: a refused call launches nothing and opens no roctx range, and its message starts with the name
 *     of the entry that was called.
 */
#ifndef DPOSER_HIP_H
#define DPOSER_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DPOSER_ABI_VERSION 1

enum {
    DPOSER_OK = 0,
    DPOSER_ERR_BAD_ARG = -1,
    DPOSER_ERR_UNSUPPORTED = -2,
    DPOSER_ERR_HIP = -3,
    DPOSER_ERR_WORKSPACE = -4
};

int dposer_abi_version(void);
const char* dposer_last_error(void);

/* ------------------------------------------------------------------------------------------
 * Score network  (lib/algorithms/advanced/model.py:93-196  class ScoreModelFC)
 * ---------------------------------------------------------------------------------------- */
typedef struct dposer_scorefc_s* dposer_scorefc_t;

/* DPOSER_PREC_BF16X3: reference-precision results ON the bf16 matrix pipe -- activations and weights are split into two bf16 terms
 * (x = hi + lo, 16 mantissa bits), every GEMM accumulates hi*hi + lo*hi + hi*lo in fp32 (three v_mfma_f32_32x32x16_bf16 per product
 * instead of sixteen-times-slower exact-fp32 MFMAs), everything outside the GEMMs (GroupNorm, SiLU, loss, optimizer, stored
 * activations) is the fp32 mode's.  hidden_dim 1024 / swish. */
enum { DPOSER_PREC_BF16 = 0, DPOSER_PREC_FP32 = 1, DPOSER_PREC_BF16X3 = 2 };
enum { DPOSER_EMB_POSITIONAL = 0, DPOSER_EMB_FOURIER = 1 };
/* config.model.nonlinearity (model.py:54-66): swish = SiLU; lrelu = LeakyReLU(0.2); elu = ELU(alpha = 1).  Swish runs on every
 * tiling; the other three on the 128-wide tilings (any batch), hidden_dim 1024 only */
enum { DPOSER_ACT_SWISH = 0, DPOSER_ACT_ELU = 1, DPOSER_ACT_RELU = 2, DPOSER_ACT_LRELU = 3 };
/* DPOSER_SDE_VE (sde_lib.py:234-292): beta_min / beta_max of dposer_sde_desc carry sigma_min / sigma_max; the network is conditioned on
 * sigma(t) (continuous VE score function, utils.py:164-181) and its output is the score itself.
 * DPOSER_SDE_VE_DISCRETE: the same SDE with the DISCRETE score function (get_score_fn(..., continuous=False), utils.py:175-181): the network is
 * conditioned on the label round((T - t) (N - 1)) -- an index into `sigmas` for scale_by_sigma and the argument of the positional embedding --
 * everything else as DPOSER_SDE_VE.  Shared-t evaluation only (sampler, Langevin step, prior loss and the two fitting loops): the training
 * loss of a discrete model is the legacy SMLD loss, the probability-flow ODE is always continuous; those entry points refuse this kind.
 * DPOSER_SDE_VP_DISCRETE: the VP SDE with its discrete score function (utils.py:157-162): label t (N - 1) and
 * score = -model / sqrt_1m_alphas_cumprod[label.long()] with the DDPM table of sde_lib.py:134-139 for THIS N (linspace(beta_min / N, beta_max / N, N),
 * cumulative product, in fp32); perturbation and reverse SDE stay the continuous ones.  Shared-t evaluation only, like the VE one. */
enum { DPOSER_SDE_SUBVP = 0, DPOSER_SDE_VP = 1, DPOSER_SDE_VE = 2, DPOSER_SDE_VE_DISCRETE = 3, DPOSER_SDE_VP_DISCRETE = 4 };

typedef struct {
    int32_t data_dim;        /* n_poses * pose_dim: 63 (axis-angle) or 126 (rot6d), 1..512  model.py:109 */
    int32_t hidden_dim;      /* 512, 1024 (the shipped configuration) or 2048: GroupNorm(32, H) groups of 16 / 32 / 64 channels  model.py:112 */
    int32_t embed_dim;       /* multiple of 128 */
    int32_t n_blocks;        /* 1..3 */
    int32_t embedding;       /* DPOSER_EMB_*      config.model.embedding_type  model.py:116-122 */
    int32_t scale_by_sigma;  /* config.model.scale_by_sigma  model.py:192 */
    int32_t num_scales;      /* length of the `sigmas` buffer  model.py:128 */
    int32_t precision;       /* DPOSER_PREC_*: bf16 MFMA (throughput), fp32 MFMA (parity) or bf16 x 3 (parity on the bf16 pipe) */
    float dropout_p;         /* config.model.dropout  model.py:113 */
    int32_t activation;      /* DPOSER_ACT_*: config.model.nonlinearity (model.py:54-66 get_act); swish is the shipped one */
} dposer_scorefc_desc;

typedef struct {             /* lib/algorithms/advanced/sde_lib.py:122-231 */
    int32_t kind;            /* DPOSER_SDE_* */
    int32_t N;               /* sde.N (mutable after construction in the reference) */
    double beta_min, beta_max, T;
} dposer_sde_desc;

int dposer_scorefc_create(const dposer_scorefc_desc* desc, dposer_scorefc_t* out);
void dposer_scorefc_destroy(dposer_scorefc_t h);

/* Flat parameter buffer: all tensors of ScoreModelFC.parameters() (model.py:98-139), in that
 * order, contiguous fp32.  The Python module keeps its nn.Parameters as views into it. */
int64_t dposer_scorefc_num_params(dposer_scorefc_t h);
int32_t dposer_scorefc_num_tensors(dposer_scorefc_t h);
int64_t dposer_scorefc_tensor_offset(dposer_scorefc_t h, int32_t idx);
int64_t dposer_scorefc_tensor_numel(dposer_scorefc_t h, int32_t idx);
/* ranges of the flat buffer that never receive a gradient (pre_dense_cond, gauss_proj.W) */
int32_t dposer_scorefc_nograd_ranges(dposer_scorefc_t h, int64_t lo[2], int64_t hi[2]);

/* Re-tile the fp32 master weights into MFMA-fragment order (bf16 or fp32) for the forward
 * GEMMs and, when with_backward != 0, transposed copies for dgrad. */
int64_t dposer_scorefc_packed_bytes(dposer_scorefc_t h, int32_t with_backward);
int dposer_scorefc_pack(dposer_scorefc_t h, const float* flat_params, void* packed, int32_t with_backward, void* stream);
/* Re-reads the A/B environment switches of the score path (DPOSER_BIG_MIN_BATCH, DPOSER_GNBWD_BIG, DPOSER_WGRAD_BIG, DPOSER_WGRAD_TR,
 * DPOSER_WGRAD_STREAM, DPOSER_WGRAD_BATCHED, DPOSER_SMALL_TILE_MAX, DPOSER_WGRAD_LAYER_LANES, DPOSER_WGRAD_GROUPS, DPOSER_FINAL_SMALL_MAX,
 * DPOSER_ADAM_WT, DPOSER_SILU_SPLIT_MAX, DPOSER_SMALL64, DPOSER_SMALL64_MIN / _MAX); they are otherwise read ONCE per process (first use),
 * never per call. */
void dposer_scorefc_tuning_reload(void);
/* TEST HOOK: dropout keep decisions of every site as bytes [n_layers][batch][hidden_dim] (device memory, NULL = back to the Philox
 * streams), used by the training epilogues of calls with exactly this batch size (hidden_dim 1024).  It lets a parity test run the
 * masks the reference drew with torch's generator through the fused training step. */
int dposer_scorefc_debug_set_dropout_masks(dposer_scorefc_t h, const unsigned char* keep, int64_t batch);

/* DPOSER_WS_GUIDED: the DPOSER_WS_TRAIN layout (every activation kept) followed by a time-bias table of n_steps rows (dposer_guided_sampler) */
enum { DPOSER_WS_INFER = 0, DPOSER_WS_SHARED_T = 1, DPOSER_WS_TRAIN = 2, DPOSER_WS_GUIDED = 3 };
int64_t dposer_scorefc_workspace_bytes(dposer_scorefc_t h, int64_t batch, int32_t mode, int32_t n_steps);
/* Which GEMM tilings and launch forms a call with `batch` samples takes under the tuning currently loaded (dposer_scorefc_tuning_reload).
 * Host only: no GPU is touched.  It runs the policy functions of the launch path itself, so a test that forces a tiling through the
 * DPOSER_* switches can assert that the forcing took.  Tilings: 0 = 256x256, 1 = 128x128, 2 = 128x32, 3 = 64x128, 4 = 64x32,
 * 5 = 128x64 (four waves), 6 = 128x64 (eight waves).
 *   plan[0] padded batch                          plan[5] tiling of the hidden x hidden weight gradients (split-K form)
 *   plan[1] GroupNorm layers, forward             plan[6] weight-gradient form: 0 split-K launches per layer, 1 one lane launch,
 *   plan[2] GroupNorm-backward dgrad                      2 one lane launch per layer group
 *   plan[3] time branch (forward and dgrad)       plan[7] number of layer groups (form 2; else 0)
 *   plan[4] post_dense / dx / sampler step        plan[8] time-branch dgrad: 0 one launch, 1 one GEMM per layer + a reduce pass
 *                                                 plan[9] parameter-gradient half on the second stream: 0 / 1
 * with_bucket_events: the plan of dposer_dsm_loss_fwd_bwd_bucketed with bucket events (data parallel).  Returns 0, or -1 with
 * dposer_last_error() set (NULL argument, batch <= 0). */
int dposer_scorefc_plan(dposer_scorefc_t h, int64_t batch, int32_t with_bucket_events, int32_t plan[10]);

/* ScoreModelFC.forward(batch, t) in eval mode -- model.py:141-196.
 *   x [B, D], labels [B] (what the reference calls `t` inside the model, i.e. t*999 from
 *   get_score_fn utils.py:152), freq [E/2] = exp(arange(E/2) * -ln(1e4)/(E/2-1)) (model.py:39-46)
 *   or gauss_proj.W for the fourier embedding, sigmas [num_scales] (model.py:128), out [B, D]. */
int dposer_scorefc_forward(dposer_scorefc_t h, const float* flat_params, const void* packed, void* ws,
                           const float* x, const float* labels, const float* freq, const float* sigmas,
                           float* out, int64_t batch, void* stream);

/* pc_sampler with the EulerMaruyama predictor, corrector 'none', optional completion imputation
 * -- lib/algorithms/advanced/sampling.py:177-188, 375-468 (score via utils.py:141-163, reverse
 * SDE sde_lib.py:75-109).  Runs loop indices [start_step, sde.N) on-device:
 *   x [B, D] in: initial state (prior sample or z), out: final x;  x_mean [B, D] out;
 *   timesteps_host [sde.N] = torch.linspace(sde.T, eps, sde.N) (sampling.py:449), HOST pointer;
 *   observation/mask [B, D] or NULL (args.task == 'completion', sampling.py:416-420);
 *   noise [n_steps][k][B][D] injected draws in the reference's draw order per step
 *     (k = 1: predictor z;  k = 3 with completion: impute-after-corrector, z, impute-after-predictor)
 *     or NULL -> in-kernel Philox4x32-10 keyed by `seed`;
 *   traj [ceil(n_steps/traj_stride)][B][D] or NULL: state after steps start+traj_stride-1, ...
 * Both time embeddings (here and in every shared-t entry point below): `freq` = the positional frequencies, or gauss_proj.W for
 * DPOSER_EMB_FOURIER (embedding of log(labels), output divided by the labels: model.py:152-155,192-194). */
int dposer_em_sampler(dposer_scorefc_t h, const float* flat_params, const void* packed, void* ws,
                      const dposer_sde_desc* sde, float* x, float* x_mean, const float* timesteps_host,
                      int32_t start_step, const float* observation, const float* mask, const float* noise,
                      uint64_t seed, float* traj, int32_t traj_stride, const float* freq, const float* sigmas,
                      int64_t batch, void* stream);

/* The same sampler with probability_flow = True: deterministic sampling along the probability-flow ODE
 * (sampling.py:182-188 with RSDE.sde of sde_lib.py:98-105), as run/demo.py:437-450 drives it to decode ODE latents:
 *   x_mean = x + (f(x, t) - 0.5 g(t)^2 score) dt,   x = x_mean   (the reference's diffusion is zeros(1)).
 * Arguments and noise layout are dposer_em_sampler's, so a trace recorded from the reference maps onto the call unchanged:
 * the predictor slot of each step is present and never read (no predictor normal is drawn); with completion the two
 * imputation slots are read (or drawn in-kernel), since the reference imputes with randn under probability flow too
 * (sampling.py:416-420).  Without observation and trajectory the call takes the one-launch-per-step fused form. */
int dposer_pf_sampler(dposer_scorefc_t h, const float* flat_params, const void* packed, void* ws,
                      const dposer_sde_desc* sde, float* x, float* x_mean, const float* timesteps_host,
                      int32_t start_step, const float* observation, const float* mask, const float* noise,
                      uint64_t seed, float* traj, int32_t traj_stride, const float* freq, const float* sigmas,
                      int64_t batch, void* stream);

/* DPoser prior: perturb -> one_step_denoise -> weighted L2 -- run/completion.py:105-149,
 * run/smplify.py:69-107, run/motion_denoising.py:99-143.  All samples share time t.
 *   x0 [B, D]; z [B, D] injected noise or NULL; x0_hat [B, D] or NULL; grad [B, D] = d loss/d x0
 *   (x0_hat is detached in the reference) or NULL; loss [1];
 *   inv_n = 1/(B*D) for torch.mean (completion.py:147), 1/batch_size for smplify.py:105. */
int dposer_prior_loss(dposer_scorefc_t h, const float* flat_params, const void* packed, void* ws,
                      const dposer_sde_desc* sde, const float* x0, const float* z, float t, int32_t weighted,
                      float inv_n, float* x0_hat, float* grad, float* loss, uint64_t seed, uint32_t step,
                      const float* freq, const float* sigmas, int64_t batch, void* stream);

/* The same evaluation with the time-bias rows of MANY steps built once: dposer_prior_table_build(t_host [n_rows]) writes the
 * table into a DPOSER_WS_SHARED_T workspace laid out for n_rows rows; dposer_prior_loss_tabled(row, table_rows = n_rows) then
 * evaluates the prior at t = t_host[row] (the caller passes the same t for the SDE scalars).  What the task loops use
 * (run/completion.py:183-201, run/motion_denoising.py:240-252 draw a new t every optimisation step). */
int dposer_prior_table_build(dposer_scorefc_t h, const float* flat_params, const void* packed, void* ws, const float* t_host,
                             int32_t n_rows, const float* freq, int64_t batch, void* stream);
/* ... with the SDE given: the rows are built for the labels the SDE's score function conditions the network on (t * 999; VE: sigma(t)).
 * sde == NULL is dposer_prior_table_build. */
int dposer_prior_table_build_sde(dposer_scorefc_t h, const float* flat_params, const void* packed, void* ws, const dposer_sde_desc* sde,
                                 const float* t_host, int32_t n_rows, const float* freq, int64_t batch, void* stream);
int dposer_prior_loss_tabled(dposer_scorefc_t h, const float* flat_params, const void* packed, void* ws, const dposer_sde_desc* sde,
                             const float* x0, const float* z, float t, int32_t row, int32_t table_rows, int32_t weighted, float inv_n,
                             float* x0_hat, float* grad, float* loss, uint64_t seed, uint32_t step, const float* sigmas,
                             int64_t batch, void* stream);

/* The prior loss on the MULTI-STEP estimate -- multi_step_denoise and the multi_denoise = True branch of the loss:
 * run/smplify.py:76-107, run/completion.py:112-149, run/motion_denoising.py:106-143, run/demo.py:251-288.  n_steps (1..64) deterministic
 * DDIM steps  noise = -score * sigma_c;  x = alpha_b / alpha_c * (x - sigma_c * noise) + sigma_b * noise  along
 *   t_traj_host [n_steps + 1], HOST: the reference's time grid linear_interpolation(t, t_end, n_steps + 1) (lib/utils/misc.py:58-61);
 * the network is evaluated at t_traj_host[0 .. n_steps - 1] (their time-bias rows built in one pass), the perturbation and the SNR of the
 * weight 0.5 sqrt(1 + alpha / sigma) (completion.py:127-128,142-145) are those of t_traj_host[0].  x0_hat [B, D] = the final state (or NULL);
 * grad = 2 w (x0 - x0_hat) inv_n (the estimate is detached) or NULL; the other arguments as dposer_prior_loss.
 * Workspace: DPOSER_WS_SHARED_T with n_steps table rows.  DPOSER_SDE_SUBVP / _VP / _VE only (this entry and dposer_prior_red_diff refuse the
 * discrete kinds: the Python surface composes those from the HIP score function). */
int dposer_prior_loss_multi(dposer_scorefc_t h, const float* flat_params, const void* packed, void* ws, const dposer_sde_desc* sde,
                            const float* x0, const float* z, const float* t_traj_host, int32_t n_steps, int32_t weighted, float inv_n,
                            float* x0_hat, float* grad, float* loss, uint64_t seed, uint32_t step, const float* freq, const float* sigmas,
                            int64_t batch, void* stream);
/* MotionDenoise.RED_Diff -- run/motion_denoising.py:145-154: perturb x0 at the shared time t, one network evaluation, then
 *   eps_pred = -score * std,  weight = sigma / alpha,  loss [1] = inv_batch * sum_b weight * sum_j (eps_pred - z)[b, j] * x0[b, j],
 *   grad [B, D] = weight * (eps_pred - z) * inv_batch  (the residual is detached in the reference), or NULL;  eps_pred [B, D] or NULL.
 * z [B, D] injected noise or NULL -> Philox(seed, step), the draws dposer_prior_loss makes.  Workspace: DPOSER_WS_SHARED_T, one row. */
int dposer_prior_red_diff(dposer_scorefc_t h, const float* flat_params, const void* packed, void* ws, const dposer_sde_desc* sde,
                          const float* x0, const float* z, float t, float inv_batch, float* eps_pred, float* grad, float* loss,
                          uint64_t seed, uint32_t step, const float* freq, const float* sigmas, int64_t batch, void* stream);

/* ---- TimeMLPs (lib/algorithms/advanced/model.py:69-90): the reference's secondary score model -------------------------------------
 *   net = Linear(in_dim, H), act, [Linear(H, H), act, Dropout(p)] x n_blocks, Linear(H, out_dim)      (in_dim = data_dim + 1: [x, t])
 * Flat parameter buffer: net.parameters() in order (weight [out][in] row-major, bias) per Linear, contiguous fp32.  Every Linear + act
 * is one MFMA GEMM launch of the score network's kernel family; the hidden width is padded to 128 channels inside the library. */
typedef struct dposer_mlp_s* dposer_mlp_t;
typedef struct {
    int32_t in_dim;          /* n_poses * pose_dim + 1 */
    int32_t out_dim;         /* n_poses * pose_dim */
    int32_t hidden_dim;      /* config.model.HIDDEN_DIM */
    int32_t n_blocks;        /* config.model.N_BLOCKS (0..8) */
    int32_t precision;       /* DPOSER_PREC_BF16 | DPOSER_PREC_FP32 */
    int32_t activation;      /* DPOSER_ACT_* (get_act, model.py:54-66) */
    float dropout_p;         /* config.model.dropout */
} dposer_mlp_desc;
int dposer_mlp_create(const dposer_mlp_desc* desc, dposer_mlp_t* out);
void dposer_mlp_destroy(dposer_mlp_t h);
int64_t dposer_mlp_num_params(dposer_mlp_t h);
int64_t dposer_mlp_packed_bytes(dposer_mlp_t h);
int64_t dposer_mlp_workspace_bytes(dposer_mlp_t h, int64_t batch);
int dposer_mlp_pack(dposer_mlp_t h, const float* flat_params, void* packed, void* stream);
/* out [B, out_dim] = net(x [B, in_dim]).  train_mode != 0: the Dropout modules draw from Philox(seed, step) (site = block index, same
 * counter layout as the score network's dropout); keep_for_backward != 0 keeps the pre-activations in `ws` for dposer_mlp_backward. */
int dposer_mlp_forward(dposer_mlp_t h, const float* flat_params, const void* packed, void* ws, const float* x, float* out, int64_t batch,
                       int32_t train_mode, int32_t keep_for_backward, uint64_t seed, uint32_t step, void* stream);
/* Backward of the forward that last ran on `ws` with keep_for_backward != 0 (same train_mode / seed / step): flat_grad [num_params]
 * (every element written; NULL: input gradient only) and dx [B, in_dim] (NULL: none). */
int dposer_mlp_backward(dposer_mlp_t h, const float* flat_params, const void* packed, void* ws, const float* dout, float* flat_grad,
                        float* dx, int64_t batch, int32_t train_mode, uint64_t seed, uint32_t step, void* stream);


/* get_sde_loss_fn.loss_fn + loss.backward() -- lib/algorithms/advanced/losses.py:80-137, 260
 * (continuous=True, reduce_mean=True, likelihood_weighting=False, model.train()).
 *   batch [B, D]; t [B] / z [B, D] injected draws or NULL (Philox: t = u*(T-eps)+eps, z ~ N(0,I));
 *   flat_grad [num_params] out: d loss / d params (no-grad ranges zeroed); loss [1] out. */
int dposer_dsm_loss_fwd_bwd(dposer_scorefc_t h, const float* flat_params, const void* packed, void* ws,
                            const dposer_sde_desc* sde, const float* batch_x, const float* t, const float* z,
                            float eps, uint64_t seed, uint32_t step, const float* freq, const float* sigmas,
                            float* flat_grad, float* loss, int64_t batch, void* stream);

/* Same step with the flat gradient delivered in BUCKETS so that the data-parallel all-reduce (RCCL, issued by the host
 * through torch.distributed) overlaps the rest of the backward pass -- the reference trains on one device
 * (run/train.py:150-170); this is the MI355X data-parallel extension BASELINE.json's north star asks for.
 *   dposer_scorefc_grad_buckets: number of buckets (n_layers + 1); [lo[b], hi[b]) are disjoint ranges of the flat buffer that
 *     cover every parameter with a gradient (the dead pre_dense_cond range, always zero in flat_grad, is in no bucket), listed in
 *     the order the backward pass completes them: last GN layer + post_dense first, ..., layer 0's weights, then layer 0's
 *     GroupNorm affine + the shared time embedding.
 *   bucket_events[b] (from dposer_event_create) is recorded on `stream` once bucket b of flat_grad is final; a
 *     communication stream waits on it with dposer_stream_wait_event before reducing that range. */
int32_t dposer_scorefc_grad_buckets(dposer_scorefc_t h, int64_t* lo, int64_t* hi, int32_t max_buckets);
int dposer_event_create(void** event);
void dposer_event_destroy(void* event);
int dposer_stream_wait_event(void* stream, void* event);
int dposer_dsm_loss_fwd_bwd_bucketed(dposer_scorefc_t h, const float* flat_params, const void* packed, void* ws,
                                     const dposer_sde_desc* sde, const float* batch, const float* t, const float* z,
                                     float eps, uint64_t seed, uint32_t step, const float* freq, const float* sigmas,
                                     float* flat_grad, float* loss, int64_t batch_size, void* const* bucket_events,
                                     int32_t n_events, void* stream);
/* The same step, telling the caller about final buckets WHILE the call is still queueing work: buckets that become final together
 * (a layer group of the backward pass: see dposer_scorefc_tuning_reload / DPOSER_WGRAD_GROUPS) are announced by ONE event --
 * bucket_events[first_bucket], recorded on `stream` -- followed at once by a call of `notify` from the calling thread with the
 * group's flat ranges (neighbouring buckets merged; n_ranges <= n_layers + 1).  The callback typically makes a communication stream
 * wait for `event` and enqueues the all-reduce of each range there: the host-side cost of issuing the collectives then overlaps
 * with GPU work that is already queued, and each collective with the rest of the backward pass.  `notify` must not synchronise
 * `stream`.  n_events >= dposer_scorefc_grad_buckets(). */
typedef void (*dposer_ranges_final_fn)(void* user, int32_t first_bucket, int32_t n_ranges, const int64_t* lo, const int64_t* hi, void* event);
int dposer_dsm_loss_fwd_bwd_notify(dposer_scorefc_t h, const float* flat_params, const void* packed, void* ws,
                                   const dposer_sde_desc* sde, const float* batch, const float* t, const float* z,
                                   float eps, uint64_t seed, uint32_t step, const float* freq, const float* sigmas,
                                   float* flat_grad, float* loss, int64_t batch_size, void* const* bucket_events,
                                   int32_t n_events, dposer_ranges_final_fn notify, void* user, void* stream);

/* Differentiable ScoreModelFC.forward for torch.autograd (model.py:141-196): forward keeps every layer
 * input / normalised activation in `ws` (DPOSER_WS_TRAIN layout); backward consumes the same `ws`.
 *   train_mode != 0: dropout active (model.train()), mask = Philox(seed, step), recomputed in backward;
 *   dout [B, D] upstream gradient; flat_grad [num_params] or NULL; dx [B, D] or NULL. */
int dposer_scorefc_forward_train(dposer_scorefc_t h, const float* flat_params, const void* packed, void* ws,
                                 const float* x, const float* labels, const float* freq, const float* sigmas,
                                 float* out, int64_t batch, int32_t train_mode, uint64_t seed, uint32_t step, void* stream);
int dposer_scorefc_backward(dposer_scorefc_t h, const float* flat_params, const void* packed, void* ws,
                            const float* labels, const float* sigmas, const float* dout, float* flat_grad, float* dx,
                            int64_t batch, int32_t train_mode, uint64_t seed, uint32_t step, void* stream);

/* optimize_fn + ema.update -- losses.py:44-58 (the lr warm-up value is computed by the caller),
 * torch.optim.Adam (losses.py:31-41), lib/algorithms/ema.py:32-51 -- ONE pass over flat fp32 buffers of n
 * elements (parameters, gradient, exp_avg, exp_avg_sq, EMA shadow).
 *   skip_lo/hi_host [n_skip <= 2]: HOST arrays of element ranges that have no gradient (Adam skipped,
 *   EMA still applied: pre_dense_cond);  grad_scale: multiplied into the gradient first (1/world_size
 *   after an all-reduce SUM);  grad_clip < 0 disables clip_grad_norm_;  adam_step = optimizer step count
 *   AFTER this update (>= 1);  ema may be NULL;  ema_one_minus_decay = 1 - min(decay, (1+n)/(10+n));
 *   scratch: >= 8 KiB floats, caller-owned and persistent across steps: scratch[0] = squared gradient norm of this step,
 *   scratch[1] = number of steps DROPPED so far because that norm was not finite (NaN / Inf gradient: parameters, moments and
 *   EMA are left untouched on the device, no host round trip; zero scratch[1] once, before the first step).
 *   Refused (DPOSER_ERR_BAD_ARG): n < 0, a no-gradient range outside 0 <= lo <= hi <= n, flat_grad not 16-byte aligned (the norm
 *   reads it four floats at a time; the other buffers need only float alignment). */
int dposer_adam_ema_clip_step(float* flat_params, const float* flat_grad, float* exp_avg, float* exp_avg_sq, float* ema,
                              int64_t n, const int64_t* skip_lo_host, const int64_t* skip_hi_host, int32_t n_skip,
                              double lr, double beta1, double beta2, double eps, double grad_clip, double grad_scale,
                              int64_t adam_step, double ema_one_minus_decay, float* scratch, void* stream);

/* Sharded optimiser step (ZeRO-1 style data parallelism): every rank owns a contiguous range of the flat buffers.
 *   dposer_grad_sqnorm: scratch[0] = sum of squares of grad[0..n) (this rank's reduce-scattered gradient range); the caller
 *   all-reduces that one float over the ranks to get the global squared norm for clip_grad_norm_ (losses.py:54-55);
 *   dposer_adam_ema_clip_step_presummed: dposer_adam_ema_clip_step on the range, taking the squared norm from scratch[0] instead
 *   of recomputing it (pointers and skip ranges are relative to the range).  grad must be 16-byte aligned in both: start every
 *   range at a multiple of 4 floats. */
int dposer_grad_sqnorm(const float* grad, int64_t n, float* scratch, void* stream);

/* Runge-Kutta stage combination on the float64 state of the probability-flow ODE (lib/algorithms/advanced/likelihood.py:86-99,
 * sampling.py:513-530 hand the state to scipy.integrate.solve_ivp, whose RK45 forms these sums on the host):
 *   out[i] = (y ? y[i] : 0) + scale * (coef[0] k[0][i] + coef[1] k[1][i] + ...), left to right in float64, no fused multiply-add.
 *   k_host / coef_host: HOST arrays of n_terms (<= 8) DEVICE pointers / coefficients; y may be NULL; out may alias nothing. */
int dposer_rk_combine_f64(double* out, const double* y, const double* const* k_host, const double* coef_host, int32_t n_terms,
                          double scale, int64_t n, void* stream);
/* Right-hand side of the probability-flow ODE around one evaluation of the score network (lib/algorithms/advanced/likelihood.py:60-65,
 * 86-95 `ode_func`; sampling.py:513-530 `ode_func`): drift = -1/2 beta(t) x - 1/2 g(t)^2 score, score = -model(x, 999 t) / std(t)
 * (sde_lib.py:100-104, utils.py:152-162), all samples at the same t, VP / sub-VP; under the VE SDE (sde_lib.py:208-253) drift =
 * -1/2 g(t)^2 score with g = sigma(t) sqrt(2 ln(sigma_max / sigma_min)), labels = sigma(t) and score = model(x, sigma(t)) (utils.py:164-175),
 * the beta terms below zero.  Two elementwise launches around the network calls:
 *   begin: x [B, D] = float(state[0 .. B*D)), labels [B] = 999 t, and -- noise != NULL, dout != NULL -- dout [B, D] = the gradient of
 *          sum(drift * noise) w.r.t. the network output (what torch.autograd hands to the network's backward in likelihood.py:29-35);
 *   end:   dstate[0 .. B*D) = double(drift(x, model_out)); with dx (the network's input gradient for `dout`) also the Hutchinson
 *          estimate dstate[B*D + b] = sum_i noise[b,i] * (dx[b,i] - 1/2 beta(t) noise[b,i]);  dx NULL: drift only (dstate [B*D]). */
int dposer_pf_ode_rhs_begin(const dposer_sde_desc* sde, float t, const double* state, const float* noise, float* x, float* labels,
                            float* dout, int64_t batch, int32_t dim, void* stream);
int dposer_pf_ode_rhs_end(const dposer_sde_desc* sde, float t, const float* x, const float* model_out, const float* dx,
                          const float* noise, double* dstate, int64_t batch, int32_t dim, void* stream);
int dposer_adam_ema_clip_step_presummed(float* flat_params, const float* flat_grad, float* exp_avg, float* exp_avg_sq, float* ema,
                                        int64_t n, const int64_t* skip_lo_host, const int64_t* skip_hi_host, int32_t n_skip,
                                        double lr, double beta1, double beta2, double eps, double grad_clip, double grad_scale,
                                        int64_t adam_step, double ema_one_minus_decay, float* scratch, void* stream);
/* the same update with torch.optim.Adam's weight_decay (losses.py:35-36 get_optimizer passes config.optim.weight_decay): the
 * clipped gradient becomes grad + weight_decay * param before the moments; presummed != 0: scratch[0] already holds the squared norm */
int dposer_adam_ema_clip_step_wd(float* flat_params, const float* flat_grad, float* exp_avg, float* exp_avg_sq, float* ema_shadow,
                                 int64_t n, const int64_t* skip_lo_host, const int64_t* skip_hi_host, int32_t n_skip, double lr,
                                 double beta1, double beta2, double eps, double weight_decay, double grad_clip, double grad_scale,
                                 int64_t adam_step, double ema_one_minus_decay, float* scratch, int32_t presummed, void* stream);
/* The same update fused with the re-packing of the weights it changes: ONE pass over the optimizer state writes parameters, moments,
 * EMA shadow AND the packed copies (MFMA fragment order, transposed dgrad copies, fp32 time-branch copies, the bias table) that the
 * next forward / backward read -- dposer_scorefc_pack at the start of the next step then has nothing to do.  `packed` must have been
 * filled by dposer_scorefc_pack(with_backward = 1) before: the zero padding of the copies is written there and never again.  All flat
 * buffers hold dposer_scorefc_num_params() floats.  Results are bitwise those of dposer_adam_ema_clip_step_wd followed by
 * dposer_scorefc_pack.  The caller owns staleness: whoever changes the parameters by other means must pack again. */
int dposer_scorefc_adam_pack_step(dposer_scorefc_t h, float* flat_params, const float* flat_grad, float* exp_avg, float* exp_avg_sq,
                                  float* ema_shadow, void* packed, const int64_t* skip_lo_host, const int64_t* skip_hi_host,
                                  int32_t n_skip, double lr, double beta1, double beta2, double eps, double weight_decay,
                                  double grad_clip, double grad_scale, int64_t adam_step, double ema_one_minus_decay, float* scratch,
                                  int32_t presummed, void* stream);

/* dposer_em_sampler restricted to the steps [start_step, start_step + n_steps) (no look-ahead imputation after the last one):
 * what a predictor-corrector loop with a corrector between the predictor calls drives (sampling.py:455-461). */
int dposer_em_sampler_steps(dposer_scorefc_t h, const float* flat_params, const void* packed, void* ws, const dposer_sde_desc* sde,
                            float* x, float* x_mean, const float* timesteps_host, int32_t start_step, int32_t n_steps,
                            const float* observation, const float* mask, const float* noise, uint64_t seed, float* traj,
                            int32_t traj_stride, const float* freq, const float* sigmas, int64_t batch, void* stream);

/* LangevinCorrector.update_fn -- sampling.py:282-302, one corrector step at a shared t (alpha = sde.alphas[timestep] for VP,
 * 1 for sub-VP, :290-294), in two phases around the batch means of :296-297:
 *   phase 0: evaluates the network at x and writes norm_sums[0] = sum_b ||grad_b||, norm_sums[1] = sum_b ||noise_b|| over this
 *            call's `batch` samples (DEVICE float[2]); under data parallelism the caller all-reduces (SUM) the two floats;
 *   phase 1: x_mean = x + step * grad, x = x_mean + sqrt(2 step) * noise, step = (snr * mean||noise|| / mean||grad||)^2 * 2 * alpha
 *            with mean = norm_sums * inv_global_batch.  Same ws for both phases, nothing else on it in between.
 * noise [B, D] injected or NULL -> Philox(seed, step) (the two phases regenerate the same numbers). */
int dposer_langevin_step(dposer_scorefc_t h, const float* flat_params, const void* packed, void* ws, const dposer_sde_desc* sde,
                         float* x, float* x_mean, float t, float alpha, float snr, const float* noise, uint64_t seed, uint32_t step,
                         float* norm_sums, int32_t phase, double inv_global_batch, const float* freq, const float* sigmas,
                         int64_t batch, void* stream);

/* get_pc_sampler.pc_sampler -- sampling.py:429-466 for EVERY registered predictor and corrector, one call: loop indices
 * [start_step, start_step + n_steps) of :455-461 (n_steps < 0: to N) are enqueued, nothing synchronises with the host, all memory is
 * the caller's.  Arguments as dposer_em_sampler_steps, plus
 *   pc               predictor (sampling.py:177-270), corrector (:273-350), corrector steps per loop index (`n_steps_each`, ignored by
 *                    corrector NONE), probability_flow (sde_lib.py:98-117), snr, and 1 / global batch for the Langevin means (:296-297);
 *   disc_table_host  N fp32 HOST entries: the SDE object's own `discrete_betas` (sub-VP / VP, sde_lib.py:136, 197) or
 *                    `discrete_sigmas` (VE, :247).  Required when the predictor or corrector reads a table (REVERSE_DIFFUSION on VP /
 *                    VE, ANCESTRAL, LANGEVIN / ALD on sub-VP / VP), else may be NULL.  alpha = 1.0f - beta; the index is
 *                    (int)((t * (float)(N - 1)) / T), as `(t * (sde.N - 1) / sde.T).long()`;
 *   norm_sums        DEVICE float[2], required for LANGEVIN.
 * Per loop index i (t = timesteps_host[i]):  corrector x n_steps_each (LANGEVIN :282-302, ALD :319-339)  ->  imputation at t
 * (:416-420, with `observation`)  ->  predictor (EULER_MARUYAMA :182-188; REVERSE_DIFFUSION :215-220 over RSDE.discretize
 * sde_lib.py:111-117 and the SDE's discretize :52-69 / :167-175 / :279-287 -- under probability_flow the score term keeps factor 1 and
 * only G is zeroed, as the reference has it; ANCESTRAL :233-253, VE / VP only and never with probability_flow; NONE :262-270)
 * ->  imputation at t  ->  trajectory entry when (i - start_step + 1) % traj_stride == 0.  x_mean on return is the last predictor's.
 * noise [n_run][(corrector != NONE ? n_steps_each : 0) + (observation ? 3 : 1)][B][D] injected draws in the reference's order
 * (corrector draws, impute-after-corrector, predictor z, impute-after-predictor; a slot the algorithm does not read is present and
 * ignored), or NULL -> Philox: STREAM_LANGEVIN at i * n_steps_each + k, STREAM_EM_NOISE at i, the imputation streams as dposer_em_sampler.
 * (EULER_MARUYAMA, NONE) is dposer_em_sampler / dposer_pf_sampler, (EULER_MARUYAMA, LANGEVIN) the bits of dposer_langevin_step +
 * dposer_em_sampler_steps.  Workspace: DPOSER_WS_SHARED_T with n_run table rows. */
enum { DPOSER_PC_PRED_NONE = 0, DPOSER_PC_PRED_EULER_MARUYAMA = 1, DPOSER_PC_PRED_REVERSE_DIFFUSION = 2, DPOSER_PC_PRED_ANCESTRAL = 3 };
enum { DPOSER_PC_CORR_NONE = 0, DPOSER_PC_CORR_LANGEVIN = 1, DPOSER_PC_CORR_ALD = 2 };
typedef struct {
    int32_t predictor;        /* DPOSER_PC_PRED_* */
    int32_t corrector;        /* DPOSER_PC_CORR_* */
    int32_t n_steps_each;     /* config.sampling.n_steps_each */
    int32_t probability_flow;
    float snr;                /* config.sampling.snr */
    double inv_global_batch;  /* LANGEVIN: 1 / (number of samples the batch means run over) */
} dposer_pc_desc;
int dposer_pc_sampler(dposer_scorefc_t h, const float* flat_params, const void* packed, void* ws, const dposer_sde_desc* sde,
                      const dposer_pc_desc* pc, float* x, float* x_mean, const float* timesteps_host, int32_t start_step,
                      int32_t n_steps, const float* observation, const float* mask, const float* noise, uint64_t seed, float* traj,
                      int32_t traj_stride, const float* disc_table_host, float* norm_sums, const float* freq, const float* sigmas,
                      int64_t batch, void* stream);

/* DPM-Solver++ (multistep, data prediction; Lu et al. 2022), orders 1 and 2: the few-step sampler.  The reference has no counterpart
 * beyond its first-order member, one step of multi_step_denoise (run/completion.py:112-129).
 * For the marginal x_t = alpha_t x_0 + sigma_t z -- (alpha, sigma) = return_alpha_sigma, sde_lib.py:177-181, :227-231, :289-292, so for
 * sub-VP sigma = 1 - exp(2 lmc) as everywhere in this library -- let lambda_t = log(alpha_t / sigma_t).  Times s_0 > s_1 > ... > s_n, state
 * x at s_0.  Step i goes from s = s_i to t = s_{i+1}, h = lambda_t - lambda_s:
 *   D_i = (x + sigma_s^2 score(x, s)) / alpha_s                                    the data prediction (completion.py:105-110)
 *   order 1:  x <- (sigma_t / sigma_s) x - alpha_t expm1(-h) D_i                    (= DDIM = one step of multi_step_denoise)
 *   order 2:  x <- (sigma_t / sigma_s) x - alpha_t expm1(-h) D_i - 1/2 alpha_t expm1(-h) (D_i - D_{i-1}) / r,
 *             r = (lambda_s - lambda_{s_{i-1}}) / h
 *   effective order at step i = min(order, i + 1), with lower_order_final also min(., n - i).
 * Every step is  x <- c_x x + c_0 D_i + c_1 D_{i-1}.  dposer_dpm_coefficients forms (c_x, c_0, c_1) in float64 on the HOST: no stream, no
 * device memory, callable without a GPU.
 *   times_host [n_steps + 1] HOST doubles, strictly decreasing, inside (0, sde.T];  coef_out [n_steps][3] HOST doubles (c_1 = 0 at
 *   effective order 1);  order 1 or 2.  DPOSER_SDE_SUBVP / _VP / _VE: the discrete kinds return DPOSER_ERR_UNSUPPORTED. */
typedef struct {
    int32_t order;              /* 1 or 2 */
    int32_t lower_order_final;  /* the last step at order 1 (what few-step grids want) */
} dposer_dpm_desc;
int dposer_dpm_coefficients(const dposer_sde_desc* sde, const double* times_host, int32_t n_steps, int32_t order,
                            int32_t lower_order_final, double* coef_out);
/* The sampler: all n_steps steps are enqueued by one call, nothing synchronises with the host, all memory is the caller's.  Per step one
 * network evaluation at s_i and one update kernel that reads the coefficients by value (the schedule above at the fp32 times widened
 * to double, rounded once to fp32).
 *   x [B, D]             in: the state at s_0, out: the state at s_n;
 *   x0_hat [B, D]        out or NULL: D_{n-1}, the last data prediction (the "denoised" sample);
 *   hist [B, D]          scratch for D_{i-1}; never read at a step of effective order 1, so it needs no initialisation; may be NULL at order 1;
 *   times_host           [n_steps + 1] HOST floats, as above; the network is evaluated at times_host[0 .. n_steps - 1];
 *   observation / mask   [B, D] or NULL (completion): the state is imputed at s_i before the evaluation at s_i,
 *                        x <- x (1 - mask) + (alpha_s observation + sigma_s z_i) mask (sampling.py:416-420 at s_i); the state returned after
 *                        the last update is NOT imputed (the caller blends observation * mask + x * (1 - mask));
 *   noise [n_steps][B][D] the draws z_i, or NULL -> Philox STREAM_IMPUTE_A keyed at i (the draw dposer_em_sampler makes ahead of its
 *                        predictor at loop index i); read only with an observation;
 *   traj [n_steps / traj_stride][B][D] or NULL: the state after step i (before the imputation at s_{i+1}) when (i + 1) % traj_stride == 0.
 * Every argument is checked before anything is launched; the discrete kinds return DPOSER_ERR_UNSUPPORTED.
 * Workspace: DPOSER_WS_SHARED_T with n_steps table rows. */
int dposer_dpm_sampler(dposer_scorefc_t h, const float* flat_params, const void* packed, void* ws, const dposer_sde_desc* sde,
                       const dposer_dpm_desc* dpm, float* x, float* x0_hat, float* hist, const float* times_host, int32_t n_steps,
                       const float* observation, const float* mask, const float* noise, uint64_t seed, float* traj, int32_t traj_stride,
                       const float* freq, const float* sigmas, int64_t batch, void* stream);

/* The MCG / DPS guided samplers for pose completion, one call: the loop of sampling.py:455-461 over
 * EulerMaruyamaPredictor.update_fn_guide (sampling.py:191-207, "this can be used to implement MCG and DPS") around
 * RSDE.sde(guide=True) (sde_lib.py:98-109).  Loop indices [start_step, start_step + n_steps) (n_steps < 0: to N) are enqueued, nothing
 * synchronises with the host, all memory is the caller's.  Arguments as dposer_em_sampler_steps (observation and mask are required), plus
 *   project          0 = DPS (the guided step alone), 1 = MCG (the guided step, then the imputation of sampling.py:416-420 at t);
 *   grad_step        the step along -d norm / d x;
 *   nonfinite_step   DEVICE int32 the caller sets to INT32_MAX: on return (after the stream has drained) the smallest loop index at
 *                    which an element of the gradient was not finite (sampling.py:203-204 raises there; this loop keeps running).
 * Per loop index i (t = timesteps_host[i], dt = -1 / N):
 *   score = score_fn(x, t): one network evaluation that keeps its activations (eval mode, no dropout);
 *   y_mean = x + (-1/2 beta x - g^2 score) dt,  y_hat = y_mean + g sqrt(-dt) z;
 *   y0 = (x + sigma^2 score) / alpha,  r = observation * mask - y0 * mask,  norm = ||r||_F over all batch * D entries of THIS call
 *   (torch.norm of the whole tensor, :201: the samples couple; no collective);
 *   grad = d norm / d x = u / alpha + J_score^T [(sigma^2 / alpha) u],  u = -mask r / norm: one dgrad-only backward through the kept
 *   activations (no weight-gradient GEMM); norm == 0 gives grad = 0, as torch's norm backward does;
 *   x = y_hat - grad_step * grad,  x_mean = y_mean;  MCG: x = x (1 - mask) + (mean_t(observation) + std_t z_imp) mask;
 *   trajectory entry when (i - start_step + 1) % traj_stride == 0.
 * The norm is a sum of per-block partials in a fixed order (no floating-point atomics): the same inputs give the same bits.
 * noise [n_run][project ? 2 : 1][B][D]: the predictor's z, then the imputation draw; NULL -> Philox STREAM_EM_NOISE at i and
 * STREAM_IMPUTE_B at i (the draws of dposer_em_sampler's predictor and of the imputation behind it).
 * DPOSER_SDE_SUBVP / DPOSER_SDE_VP (continuous score function).  `packed` must hold the backward copies (with_backward = 1).
 * Workspace: DPOSER_WS_GUIDED with n_run table rows. */
int dposer_guided_sampler(dposer_scorefc_t h, const float* flat_params, const void* packed, void* ws, const dposer_sde_desc* sde,
                          float* x, float* x_mean, const float* timesteps_host, int32_t start_step, int32_t n_steps,
                          const float* observation, const float* mask, const float* noise, uint64_t seed, float* traj,
                          int32_t traj_stride, int32_t project, float grad_step, int32_t* nonfinite_step, const float* freq,
                          const float* sigmas, int64_t batch, void* stream);

/* DPoserComp.optimize -- run/completion.py:167-207 (loss :131-149, weights :151-155): `n_steps` Adam steps on the pose batch
 * x [B, D] (in: the initial value, i.e. the observation; out: the optimised variable -- the caller applies the final
 * observation/mask blend of :205) under  w_prior[i] * mean(w (x - x0_hat)^2) + w_data[i] * MSE(x * mask, obs * mask).
 *   adam_m / adam_v [B, D]: torch.optim.Adam moments, zero on entry for a fresh optimiser (per-sample state: the loop shards
 *   over GPUs with no collective);  t_host / weighted_host / w_prior_host / w_data_host [n_steps]: HOST arrays of the
 *   per-step time, the `weighted` flag (the reference passes quan_t there, :196) and the loss weights;
 *   noise [n_steps, B, D] injected z of :133, or NULL -> Philox(seed, step0 + i).  Workspace: DPOSER_WS_SHARED_T with
 *   n_steps table rows. */
int dposer_completion_optimize(dposer_scorefc_t h, const float* flat_params, const void* packed, void* ws, const dposer_sde_desc* sde,
                               float* x, const float* observation, const float* mask, float* adam_m, float* adam_v,
                               const float* t_host, const int32_t* weighted_host, const float* w_prior_host, const float* w_data_host,
                               int32_t n_steps, double lr, double beta1, double beta2, double eps, const float* noise, uint64_t seed,
                               uint32_t step0, const float* freq, const float* sigmas, int64_t batch, void* stream);

/* Per-launch GEMM timing (HIP events recorded on the launch stream around every MFMA GEMM launch; off by
 * default).  collect() synchronises the recorded events and returns, per kernel kind, the summed
 * duration [ms], launch count and algorithmic FLOPs (2*M*N*K of the un-padded problem); arrays of
 * dposer_profile_num_kinds() entries in HOST memory.  Used by bench.py for the live roofline.
 * enable(on): 0 = off (and forget the records), -1 = pause (keep them), 1 = every GEMM launch, 2 + k = launches of epilogue kind k only (k: 0 gn_fwd, 1 gn_fwd_train,
 * 2 bias_silu, 3 rowmajor, 4 plain_ft, 5 gn_bwd_dgrad, 6 silu_bwd_dgrad, 7 wgrad, 8 post_em_step) -- two event records per
 * launch cost about 3 % of a training step when every launch is bracketed, so a timed region brackets one kind. */
void dposer_profile_enable(int32_t on);
int32_t dposer_profile_num_kinds(void);
int dposer_profile_collect(double* ms_host, int64_t* launches_host, double* flops_host);
void dposer_profile_kind_name(int32_t kind, char* out, int32_t n);

/* ------------------------------------------------------------------------------------------
 * Body model  (lib/body_model/body_model.py:68-112 -> smplx.lbs, lib/utils/transforms.py:227-235)
 * ---------------------------------------------------------------------------------------- */
/* rot6d_to_mat3x3 -- lib/utils/transforms.py:227-235: rot6d [n, 6] -> rotmat [n, 3, 3] */
int dposer_rot6d_to_rotmat(const float* rot6d, float* rotmat, int64_t n, void* stream);
/* batch_rodrigues -- smplx/lbs.py: axis-angle [n, 3] -> rotmat [n, 3, 3] */
int dposer_rodrigues(const float* axis_angle, float* rotmat, int64_t n, void* stream);

/* rot6d_to_axis_angle -- lib/utils/transforms.py:197-224 (Gram-Schmidt, then torchgeometry.rotation_matrix_to_angle_axis:
 * matrix -> unit quaternion -> angle-axis with the angle in [0, pi]; NaNs zeroed as :223); also from a rotation matrix [n, 3, 3] */
int dposer_rot6d_to_axis_angle(const float* rot6d, float* axis_angle, int64_t n, void* stream);
int dposer_rotmat_to_axis_angle(const float* rotmat, float* axis_angle, int64_t n, void* stream);

typedef struct dposer_body_s* dposer_body_t;
typedef struct {
    int32_t num_joints;      /* 24 SMPL / 52 SMPL-H / 55 SMPL-X */
    int32_t num_vertices;
    int32_t num_shape;       /* betas + expression coefficients */
    int32_t num_extra;       /* vertex-selected extra joints */
    int32_t num_landmarks;   /* barycentric landmarks */
} dposer_body_desc;
int dposer_body_create(const dposer_body_desc* desc, const int32_t* parents_host, dposer_body_t* out);
void dposer_body_destroy(dposer_body_t h);

/* Rest shape: shape blend shapes + joint regression -- smplx/lbs.py blend_shapes + vertices2joints at the head of lbs(), as
 * reached from lib/body_model/body_model.py:75-88 with betas / expression given per pose (run/smplify.py:200-260 optimises
 * betas; the task loops pass constant ones).
 *   v_shaped[b] = v_template + shapedirs . shape[b]          shapedirs [V*3, L] (the asset's [V,3,L]), shape [B, L]
 *   j_rest[b]   = J_regressor @ v_shaped[b] = j_template + jdirs . shape[b]
 * The regressor is LINEAR, so it is applied once to the template and to every blend-shape direction on the host side
 * (j_template [J*3] = J_regressor @ v_template, jdirs [J*3, L] = J_regressor @ shapedirs[..., l]); per pose the joints are an
 * L-term combination instead of a [J, V] x [V, 3] product.
 * Backward: d_shape [B, L] = d_v_shaped . shapedirs + d_j_rest . jdirs; scratch >= dposer_shape_blend_scratch_floats(...) floats. */
int dposer_shape_blend_forward(const float* v_template, const float* shapedirs, const float* j_template, const float* jdirs,
                               const float* shape, float* v_shaped, float* j_rest, int32_t num_vertices, int32_t num_joints,
                               int32_t num_shape, int64_t batch, void* stream);
int64_t dposer_shape_blend_scratch_floats(int32_t num_vertices, int32_t num_shape, int64_t batch);
int dposer_shape_blend_backward(const float* shapedirs, const float* jdirs, const float* d_v_shaped, const float* d_j_rest,
                                float* d_shape, float* scratch, int32_t num_vertices, int32_t num_joints, int32_t num_shape,
                                int64_t batch, void* stream);

/* Forward kinematics: Rodrigues + kinematic chain (smplx/lbs.py batch_rodrigues, batch_rigid_transform)
 * with the pose assembled as SMPLX.forward does (reference call site lib/body_model/body_model.py:75-88):
 *   pose_segments_host[i]: DEVICE pointer to segment i, [B, segment_joints[i]*3] axis-angle, or NULL
 *     (= zeros, what the reference gets from the module's default parameters); the host arrays
 *     themselves are HOST memory.  SMPL-X order: global(1) body(21) jaw(1) leye(1) reye(1) lhand(15) rhand(15).
 *   j_rest [J,3] (shared) or [B,J,3]: rest-pose joints (J_regressor @ v_shaped);
 *   joints [B, n_out, 3] out: posed joints [0, n_out) (+ transl [B,3] if not NULL);
 *   rel_transforms [B, n_out, 12] out or NULL: rows of the 3x4 skinning transforms A_i. */
int dposer_fk_joints(dposer_body_t h, const float* const* pose_segments_host, const int32_t* segment_joints_host,
                     int32_t num_segments, const float* j_rest, int32_t j_rest_batched, const float* transl,
                     float* joints, float* rel_transforms, int32_t n_out, int64_t batch, void* stream);

/* Gradient of dposer_fk_joints with respect to the pose segments and the rest joints, given the gradient with respect to the
 * posed joints -- the chain rule over the n_out joints alone: no vertex, no skinning, no blend GEMM (the LBS backward needs more
 * than 125 KB per pose for the vertices; this call reads and writes 60 bytes per joint and pose of workspace besides its arguments).
 *   pose_segments_host / segment_joints_host / j_rest / j_rest_batched: as in dposer_fk_joints (the same values as in the forward call);
 *   d_joints [B][d_joints_ld] floats, d_joints_ld >= 3 * n_out: the first 3 * n_out of a row are the gradient with respect to the
 *     posed joints [0, n_out);
 *   d_pose_segments_host[i]: DEVICE pointer to [B, segment_joints[i]*3] or NULL (not wanted); the axis-angle gradient of segment i
 *     is written there, with zeros for joints >= n_out;
 *   d_jrest [B, n_out, 3] out or NULL: the gradient with respect to the rest joints [0, n_out) of every pose (a caller with shared
 *     rest joints sums over the batch);
 *   workspace: >= dposer_fk_joints_backward_workspace_bytes(h, n_out, batch) bytes, 16-byte aligned, caller-owned; contents are
 *     scratch (the forward's transforms [B][n_out][12] and posed joints).
 * The translation's gradient is the sum of d_joints over the joints and stays with the caller.  Rotations are those of
 * dposer_fk_joints (rodrigues with smplx's + 1e-8) and rodrigues_bwd.  One lane walks one pose's chain from the last joint to the
 * root and a parent adds its children in descending joint order: one fixed summation order, the same bits for the same inputs.
 * Every argument is checked before the first launch; no allocation, no synchronisation. */
int64_t dposer_fk_joints_backward_workspace_bytes(dposer_body_t h, int32_t n_out, int64_t batch);
int dposer_fk_joints_backward(dposer_body_t h, const float* const* pose_segments_host, const int32_t* segment_joints_host,
                              int32_t num_segments, const float* j_rest, int32_t j_rest_batched, const float* d_joints,
                              int64_t d_joints_ld, int32_t n_out, float* const* d_pose_segments_host, float* d_jrest,
                              void* workspace, int64_t batch, void* stream);

/* The joint-residual stage of a 3D-joint measurement on a normalised body pose: what a sampler or a fitting loop guided by observed 3D
 * joints evaluates once per step.  Per pose b:
 *   pose = denormalise(y0[b]),  y0 [B, 63]: 21 body joints, axis-angle, in the network's normalised space;
 *     norm_mode / norm_a / norm_b exactly as in dposer_motion_denoise_args: 0 none / 1 z-score (mean, std) / 2 min-max (min, max), [63];
 *   J = the 22 posed joints of dposer_fk_joints over (root_orient [B,3] or NULL = identity, pose, every other joint at rest), rest joints
 *     j_rest [J,3] or [B,J,3] (j_rest_batched), + transl [B,3] if not NULL;  `body` is any supported tree (its first 22 joints are the body).
 * The observation rule is the motion-denoising one (PARTIAL OBSERVATIONS below), restated:
 *   joints_obs [B, n_obs, 3];  joints_conf [B, n_obs] or NULL = 1;  obs_rows DEVICE [n_obs]: distinct tree joints in [0, 22), or NULL =
 *   0 .. n_obs-1 (the caller checks range and distinctness; a row outside [0, 22) counts as not live and is never dereferenced);
 *   an entry is LIVE iff c > 0 -- false for 0, for negatives and for NaN;  a dead entry's observation may be NaN or Inf and never
 *   enters a sum.
 * Outputs:
 *   s[b] = sum_live c |J[rows[j]] - o_j|^2            [B]
 *   v[b] = 1/2 d s[b] / d y0[b]                        [B, 63]: FK forward, residual, the reverse walk of dposer_fk_joints_backward, the
 *                                                      normaliser's scale.  A pose without a live entry gets s = 0, v = 0.
 * fp32 throughout; one lane sums a pose's entries in ascending column order and walks its chain: the same inputs give the same bits.
 * data_dim must be 63: a rot6d network (126) returns DPOSER_ERR_UNSUPPORTED.  n_obs in 1..22.  scratch: caller-owned,
 * >= dposer_joint_guide_stage_scratch_bytes(batch), 16-byte aligned.  Every argument is checked before the first launch; no allocation,
 * no synchronisation. */
int64_t dposer_joint_guide_stage_scratch_bytes(int64_t batch);
int dposer_joint_guide_stage(dposer_body_t body, const float* y0, int32_t data_dim, int32_t norm_mode, const float* norm_a,
                             const float* norm_b, const float* root_orient, const float* transl, const float* j_rest,
                             int32_t j_rest_batched, const float* joints_obs, const float* joints_conf, const int32_t* obs_rows,
                             int32_t n_obs, float* s, float* v, void* scratch, int64_t batch, void* stream);

/* DPS on observed 3D joints, every step in one call: dposer_guided_sampler's loop with the stage above, dposer_joint_guide_stage, as the
 * measurement operator instead of a pose-space mask.  Arguments: those of dposer_guided_sampler without
 * observation / mask / project; the stage's inputs (body .. n_obs, same meaning, same observation rule); norm_scope; a caller-owned
 * scratch of >= dposer_joint_guided_scratch_bytes(B) bytes, 16-byte aligned.  Per loop index i, t = timesteps_host[i], dt = -1/N, in the
 * notation of dposer_guided_sampler's contract:
 *   score = score_fn(x, t) with kept activations;  y_mean, y_hat as above;  y0 = (x + sigma^2 score) / alpha;
 *   (s[b], v[b]) = the stage at y0:  s[b] = sum_live c |J_rows[j](denormalise(y0[b])) - o_j|^2,  v[b] = 1/2 d s[b] / d y0[b];
 *   norm_scope 0 ("batch"):  norm = sqrt(sum_b s[b]), the reference's torch.norm over the whole tensor (sampling.py:201), the sum taken
 *     by one block in a fixed order;   norm_scope 1 ("sample"):  norm_b = sqrt(s[b]) -- every row is its own problem and its
 *     guidance does not depend on its batch mates;
 *   grad = (v / alpha + J_score^T [(sigma^2 / alpha) v]) / norm   (the dgrad's upstream gradient is written without the 1 / norm, as
 *     k_guided_resid does);  norm == 0 gives grad = 0: a row (scope 1) or a batch (scope 0) without a live entry is sampled unconditionally;
 *   x = y_hat - grad_step grad,  x_mean = y_mean.
 * Trajectory slots and nonfinite_step behave as in dposer_guided_sampler (a NaN observation under a positive confidence raises the
 * flag at its loop index).  noise [n_run][1][B][D] or NULL = Philox STREAM_EM_NOISE at i.  No MCG projection: there is no pose-space
 * mask.  Workspace DPOSER_WS_GUIDED with n_run table rows; `packed` holds the backward copies.  Continuous sub-VP and VP only: VE and the
 * discrete kinds return DPOSER_ERR_UNSUPPORTED, and so does a network whose data_dim is not 63 (rot6d: 126).  Every argument is checked
 * before anything is launched; no allocation, no synchronisation. */
int64_t dposer_joint_guided_scratch_bytes(int64_t batch);
int dposer_joint_guided_sampler(dposer_scorefc_t h, const float* flat, const void* packed, void* ws, const dposer_sde_desc* sde, float* x,
                                float* x_mean, const float* timesteps_host, int32_t start_step, int32_t n_steps, dposer_body_t body,
                                int32_t norm_mode, const float* norm_a, const float* norm_b, const float* root_orient, const float* transl,
                                const float* j_rest, int32_t j_rest_batched, const float* joints_obs, const float* joints_conf,
                                const int32_t* obs_rows, int32_t n_obs, int32_t norm_scope, const float* noise, uint64_t seed, float* traj,
                                int32_t traj_stride, float grad_step, int32_t* nonfinite_step, void* scratch, const float* freq,
                                const float* sigmas, int64_t B, void* stream);

/* The keypoint-residual stage of a 2D-keypoint measurement on a normalised body pose: dposer_joint_guide_stage with a pinhole camera and
 * SMPLify's robust reprojection residual (lib/body_model/fitting_losses.py:6-47 perspective_projection + gmof, :69-75 the weighted
 * residual of body_fitting_loss) in place of the 3D distance.  body .. j_rest_batched, obs_rows, n_obs, s, v, scratch, batch, stream: the
 * contract of dposer_joint_guide_stage, word for word.  transl [B,3] or NULL is the CAMERA translation: FK adds it to the posed joints,
 * exactly as SMPLify passes transl = camera_t to the body model (perspective_projection never adds its `translation` argument, and the
 * camera rotation is the identity: fitting_losses.py:69).  The camera and the observation:
 *   keypoints [B, n_obs, 2] pixels;  keypoints_conf [B, n_obs] or NULL = 1;
 *   focal  DEVICE [B]: one focal length per pose, pixels (a caller with one camera fills the vector);  center DEVICE [B, 2] pixels;
 *   sigma: the Geman-McClure scale in pixels, <= 0 = no robustifier; a positive sigma outside [1e-18, 1e18] (its square is no normal float)
 *     and NaN are refused;   z_near > 0, finite: the nearest depth that projects, metres.
 * Per pose b and column j, with (X, Y, Z) = posed joint rows[j]:
 *   LIVE iff c > 0 (false for 0, negatives and NaN) AND Z > z_near (false for NaN).  A dead entry's keypoint may be NaN or Inf and never
 *     enters a sum.  A joint at or behind z_near is dead for this evaluation, in s and in v alike; it is not an error.
 *   ru = focal (X / Z) - (k_u - center_u),  rv = focal (Y / Z) - (k_v - center_v): the centre is taken off the observation, not added to
 *     the projection, so that no pair of numbers hundreds of pixels large is subtracted;
 *   rho(r) = sigma^2 r^2 / (sigma^2 + r^2)  (gmof),  or r^2 for sigma <= 0;
 *   s[b] = sum_live c^2 (rho(ru) + rho(rv))           [B]      (the weight is the reference's joints_conf ** 2, not the 3D stage's c)
 *   v[b] = 1/2 d s[b] / d y0[b]                        [B, 63]: FK forward, residual and its gradient on the 22 posed joints (one lane per
 *                                                      pose, zeros for unobserved rows, columns in ascending order), the reverse walk of
 *                                                      dposer_fk_joints_backward, the normaliser's scale.  No live entry: s = 0, v = 0.
 * The 22 tree joints only: the extra joints SMPLify reads from vertices (nose, eyes, ears, toes) are not observed here.
 * fp32 throughout; the same inputs give the same bits.  data_dim must be 63: a rot6d network (126) returns DPOSER_ERR_UNSUPPORTED.
 * scratch: caller-owned, >= dposer_keypoint_guide_stage_scratch_bytes(batch), 16-byte aligned.  Every argument is checked before the first
 * launch; no allocation, no synchronisation. */
int64_t dposer_keypoint_guide_stage_scratch_bytes(int64_t batch);
int dposer_keypoint_guide_stage(dposer_body_t body, const float* y0, int32_t data_dim, int32_t norm_mode, const float* norm_a,
                                const float* norm_b, const float* root_orient, const float* transl, const float* j_rest,
                                int32_t j_rest_batched, const float* keypoints, const float* keypoints_conf, const int32_t* obs_rows,
                                int32_t n_obs, const float* focal, const float* center, float sigma, float z_near, float* s, float* v,
                                void* scratch, int64_t batch, void* stream);

/* DPS on observed 2D keypoints, every step in one call: dposer_joint_guided_sampler's loop -- the same launches around the stage -- with
 * dposer_keypoint_guide_stage as the measurement: K bodies that reproject onto the same keypoints and differ in depth.  Arguments: those
 * of dposer_joint_guided_sampler with the keypoint stage's observation block (keypoints .. z_near) in place of joints_obs / joints_conf;
 * norm_scope, trajectory slots, nonfinite_step (a NaN keypoint under a positive confidence raises it at its loop index), noise injection
 * and the Philox stream are the same.  Liveness is decided anew at every index: a joint that y0 puts at or behind z_near does not guide
 * that index.  scratch >= dposer_keypoint_guided_scratch_bytes(B) bytes, 16-byte aligned.  Continuous sub-VP and VP only, D = 63 only:
 * everything else returns DPOSER_ERR_UNSUPPORTED.  Every argument is checked before anything is launched; no allocation, no
 * synchronisation. */
int64_t dposer_keypoint_guided_scratch_bytes(int64_t batch);
int dposer_keypoint_guided_sampler(dposer_scorefc_t h, const float* flat, const void* packed, void* ws, const dposer_sde_desc* sde, float* x,
                                   float* x_mean, const float* timesteps_host, int32_t start_step, int32_t n_steps, dposer_body_t body,
                                   int32_t norm_mode, const float* norm_a, const float* norm_b, const float* root_orient, const float* transl,
                                   const float* j_rest, int32_t j_rest_batched, const float* keypoints, const float* keypoints_conf,
                                   const int32_t* obs_rows, int32_t n_obs, const float* focal, const float* center, float sigma, float z_near,
                                   int32_t norm_scope, const float* noise, uint64_t seed, float* traj, int32_t traj_stride, float grad_step,
                                   int32_t* nonfinite_step, void* scratch, const float* freq, const float* sigmas, int64_t B, void* stream);

/* Linear blend skinning -- smplx/lbs.py lbs() + SMPLX.forward joint assembly, as called from
 * lib/body_model/body_model.py:75-103 (BodyModel.forward) and lib/body_model/smpl.py:67-77.
 *   posedirs_packed: dposer_lbs_pack_posedirs(posedirs [(J-1)*9, V*3]) (MFMA fragment order, fp32);
 *   v_shaped [V,3] (betas folded in, shared) or [B,V,3]; j_rest as in dposer_fk_joints;
 *   skin_idx / skin_w [V, skin_k]: ELL form of lbs_weights [V,J] (zero weights dropped or padded);
 *   extra_vertex_ids [num_extra], lmk_tri [num_landmarks,3] (= faces[lmk_faces_idx]), lmk_bary [num_landmarks,3] -- or all three NULL: the rows behind
 *   the kinematic tree's J joints are then left unwritten (callers that read tree joints only: the motion-denoising loop);
 *   verts [B,V,3] out; joints [B, J+num_extra+num_landmarks, 3] out (SMPL-X: 55+21+51 = 127). */
int64_t dposer_lbs_posedirs_packed_bytes(dposer_body_t h);
int dposer_lbs_pack_posedirs(dposer_body_t h, const float* posedirs, void* packed, void* stream);
int64_t dposer_lbs_workspace_bytes(dposer_body_t h, int64_t batch);
int dposer_lbs_forward(dposer_body_t h, void* ws, const void* posedirs_packed, const float* const* pose_segments_host,
                       const int32_t* segment_joints_host, int32_t num_segments, const float* j_rest, int32_t j_rest_batched,
                       const float* v_shaped, int32_t v_shaped_batched, const int32_t* skin_idx, const float* skin_w,
                       int32_t skin_k, const float* transl, const int32_t* extra_vertex_ids, const int32_t* lmk_tri,
                       const float* lmk_bary, float* verts, float* joints, int64_t batch, void* stream);

/* dposer_lbs_forward for callers that need the vertices ONLY for the temporal smoothness term of run/motion_denoising.py:253-255
 * (`torch.mean(torch.norm(verts[:-1] - verts[1:], dim=-1))` and its autograd): skinning and that term's gradient in one pass, the
 * vertices never reach HBM.  batch = whole sequences of frames_per_sequence consecutive frames (neighbours never cross a sequence);
 *   d_verts [B,V,3] out = scale * (u_t - u_{t-1}), u_t = (v[t] - v[t+1]) / ||v[t] - v[t+1]|| (0/0 = NaN like torch's sqrt backward);
 *   dist_part [B, ceil(V/256)] out: sums of ||v[t] - v[t+1]|| over blocks of 256 vertices (0 for the last frame of a sequence) --
 *   their sum / ((F-1) V) is the term's value;  joints [B, J+num_extra+num_landmarks, 3]: only [:, :J] is written (the extra
 *   vertices / landmarks would need the vertices).  skin_k must be 4.  Other arguments as dposer_lbs_forward. */
int dposer_lbs_forward_temporal_grad(dposer_body_t h, void* ws, const void* posedirs_packed, const float* const* pose_segments_host,
                                     const int32_t* segment_joints_host, int32_t num_segments, const float* j_rest, int32_t j_rest_batched,
                                     const float* v_shaped, int32_t v_shaped_batched, const int32_t* skin_idx, const float* skin_w,
                                     int32_t skin_k, const float* transl, int64_t frames_per_sequence, float scale, float* d_verts,
                                     float* dist_part, float* joints, int64_t batch, void* stream);

/* The same step with NO vertex-sized array in HBM at all (round 6; run/motion_denoising.py:217-218,253-267):
 *   dposer_lbs_forward_front          FK + pose-blend offsets of dposer_lbs_forward without its skinning kernel: joints[:, :J] and the
 *                                     workspace `ws` (pose feature, skinning transforms, offsets);
 *   dposer_lbs_backward_temporal      dposer_lbs_backward whose vertex gradient is the temporal term's -- scale * (u_t - u_{t-1}) -- formed
 *                                     inside the skinning-backward kernel from `ws_fwd` (the vertices of a frame and of its two neighbours
 *                                     are skinned in registers); d_joints carries the data term.  dist_part4 [B, ceil(V/256), 4] out: per-wave
 *                                     sums of ||v[t] - v[t+1]||, ((p0 + p1) + p2) + p3 of an entry = dist_part of dposer_lbs_forward_temporal_grad.
 *                                     The vertices and the vertex gradient carry the bits of dposer_lbs_forward + the two-kernel gradient; the backward half agrees with
 *                                     dposer_lbs_backward to fp32 rounding (FMA-contracted transform blend: 2e-6 on the optimised poses).
 *   dposer_lbs_temporal_in_backward_ok(h, skin_k, batch): 1 when dposer_lbs_backward_temporal can run (prepared joint lists with the
 *                                     matrix-pipe tables, four influences per vertex, batch >= DPOSER_LBS_JOINT_STREAM_MIN, bf16 x 3 blend);
 *                                     dposer_motion_denoise_optimize asks it and falls back to the forms above. */
int32_t dposer_lbs_temporal_in_backward_ok(dposer_body_t h, int32_t skin_k, int64_t batch);
int dposer_lbs_forward_front(dposer_body_t h, void* ws, const void* posedirs_packed, const float* const* pose_segments_host,
                             const int32_t* segment_joints_host, int32_t num_segments, const float* j_rest, int32_t j_rest_batched,
                             const float* transl, float* joints, int64_t batch, void* stream);
int dposer_lbs_backward_temporal(dposer_body_t h, const void* ws_fwd, void* ws_bwd, const void* posedirs_bwd_packed,
                                 const float* const* pose_segments_host, const int32_t* segment_joints_host, int32_t num_segments,
                                 const float* j_rest, int32_t j_rest_batched, const float* v_shaped, int32_t v_shaped_batched,
                                 const int32_t* skin_idx, const float* skin_w, int32_t skin_k, const int32_t* joint_ptr,
                                 const int32_t* joint_vidx, const float* joint_w, int64_t frames_per_sequence, float scale,
                                 float* dist_part4, const float* d_joints, int64_t d_joints_ld, float* const* d_pose_segments_host,
                                 int64_t batch, void* stream);

/* Pose-pair errors -- Evaler.eval_bodys / multi_eval_bodys of lib/dataset/AMASS.py:275-316 for `batch` samples, each one reference
 * body and `hypotheses` hypothesis bodies, in one call: MPVPE (mean per-vertex position error) and MPJPE (mean per-joint position
 * error) per hypothesis and their minimum over the hypotheses.  No vertex array exists in memory: both bodies are skinned in registers
 * from the workspaces two dposer_lbs_forward_front calls left behind.
 * Inputs:
 *   ws_ref / joints_ref: workspace and joints [batch, J + num_extra + num_landmarks, 3] of the front call over the `batch` reference poses
 *   (only joints[:, :J] is valid, as that call leaves it);  ws_hyp / joints_hyp: the same of ONE front call over batch * hypotheses poses,
 *   hypothesis h of sample b at row b * hypotheses + h.  Both workspaces unmodified since.
 *   v_shaped [V,3] (shared) or [batch,V,3] (sample b's, shared by its hypotheses); skin_idx / skin_w / skin_k as dposer_lbs_forward;
 *   transl_ref [batch,3] / transl_hyp [batch * hypotheses,3] or NULL: the translations the two front calls were given;
 *   vert_list [num_listed_vertices] int32 or NULL (= all V vertices); joint_rows [num_listed_rows] int32 (at most 4096) or NULL (= all
 *   J + num_extra + num_landmarks rows of the LBS joint output); max_listed_row: the largest entry of joint_rows (ignored when it is NULL);
 *   extra_vertex_ids / lmk_tri / lmk_bary as dposer_lbs_forward: required when max_listed_row reaches the rows they produce.
 *   The lists are device arrays and are NOT range-checked: the caller guarantees 0 <= vert_list[i] < V and
 *   0 <= joint_rows[i] <= max_listed_row < J + num_extra + num_landmarks.
 * Rule, for sample b and hypothesis h:
 *   mpvpe_h[b,h] = scale * (sum over listed vertices of ||v_hyp - v_ref||) / num_listed_vertices.  Both vertices are formed exactly as
 *   dposer_lbs_forward forms them: p = v_shaped + offsets, T = sum_k w_k A[j_k], v = T [p ; 1] + transl, the blend and the product
 *   contracted to FMAs as in its skinning kernels.  Differences, squares, their sum x^2 + y^2 + z^2 (left to right), the square root
 *   (correctly rounded), the sums, the division and the scaling are fp32 without contraction.
 *   mpjpe_h[b,h] is the same over the listed joint rows: a row < J is read from the two joint arrays; a row in [J, J + num_extra) is the
 *   skinned vertex extra_vertex_ids[row - J] of either body; a landmark row l is ((0 + v_0 w_0) + v_1 w_1) + v_2 w_2 over the skinned
 *   vertices lmk_tri[l] with weights lmk_bary[l], per coordinate (dposer_lbs_forward's landmark sum).
 *   mpvpe[b] = min_h mpvpe_h[b,h], mpjpe[b] = min_h mpjpe_h[b,h]; a NaN value makes the minimum NaN (torch.min).  min_into = 0 writes
 *   mpvpe / mpjpe; min_into = 1 takes the minimum of the new values and what the two arrays already hold (a NaN on either side
 *   stays): hypotheses can be scored in several calls against a bounded workspace.
 * Summation order: the vertex distances of a 256-entry block of the list are added by xor butterfly inside each of four 64-lane waves,
 *   the four waves as ((p0 + p1) + p2) + p3, the blocks in list order; the joint distances by 128 strided per-thread sums, a butterfly per
 *   wave, then wave 0 + wave 1.  No atomics.  The order depends on the list lengths alone: a sample's outputs are a function of its own
 *   data, whatever the batch, its position in it, the number of hypotheses or their split into calls.
 * Outputs: mpvpe [batch], mpjpe [batch]; mpvpe_h / mpjpe_h [batch, hypotheses] or NULL.
 * scratch: dposer_pose_pair_errors_scratch_bytes(body, batch, hypotheses, listed_vertices) bytes (listed_vertices <= 0: all vertices),
 *   256-byte aligned.  Queues two kernels on the stream; allocates nothing, never synchronises the host.
 * Layout (LP64): pointers and int64 at 8-byte alignment, int32 / float at 4; sizeof = 200. */
typedef struct dposer_pose_pair_errors_args {
    dposer_body_t body;               /*   0 */
    const void* ws_ref;               /*   8 */
    const void* ws_hyp;               /*  16 */
    const float* joints_ref;          /*  24 */
    const float* joints_hyp;          /*  32 */
    const float* v_shaped;            /*  40 */
    int32_t v_shaped_batched;         /*  48 */
    int32_t skin_k;                   /*  52 */
    const int32_t* skin_idx;          /*  56 */
    const float* skin_w;              /*  64 */
    const float* transl_ref;          /*  72 */
    const float* transl_hyp;          /*  80 */
    const int32_t* vert_list;         /*  88 */
    const int32_t* joint_rows;        /*  96 */
    int32_t num_listed_vertices;      /* 104 */
    int32_t num_listed_rows;          /* 108 */
    int32_t max_listed_row;           /* 112 */
    int32_t hypotheses;               /* 116 */
    const int32_t* extra_vertex_ids;  /* 120 */
    const int32_t* lmk_tri;           /* 128 */
    const float* lmk_bary;            /* 136 */
    int64_t batch;                    /* 144 */
    float scale;                      /* 152: 1000 = millimetres, 100 = centimetres for bodies in metres */
    int32_t min_into;                 /* 156 */
    float* mpvpe;                     /* 160 */
    float* mpjpe;                     /* 168 */
    float* mpvpe_h;                   /* 176 */
    float* mpjpe_h;                   /* 184 */
    void* scratch;                    /* 192 */
} dposer_pose_pair_errors_args;
int64_t dposer_pose_pair_errors_scratch_bytes(dposer_body_t h, int64_t batch, int32_t hypotheses, int32_t listed_vertices);
int dposer_pose_pair_errors(const dposer_pose_pair_errors_args* args, void* stream);

/* Backward of dposer_lbs_forward (autograd of BodyModel.forward w.r.t. pose / rest joints / v_posed; the reference
 * differentiates through smplx in run/motion_denoising.py:217-218,255-267 and run/smplify.py:200-260).
 *   ws_fwd: the workspace of the matching forward call (unmodified since);  posedirs_bwd_packed:
 *   dposer_lbs_pack_posedirs_bwd(posedirs);  joint_ptr [J+1] / joint_vidx / joint_w: CSR-by-joint form of lbs_weights;
 *   d_verts [B,V,3]; d_joints [B, d_joints_ld] (first J*3 entries of a row = gradient of the posed LBS joints; extras and
 *   landmarks are vertex gathers and must be folded into d_verts by the caller);
 *   d_pose_segments_host[i]: DEVICE pointer [B, seg_joints*3] out or NULL;  d_jrest [B,J,3] out or NULL;
 *   d_vposed [B,V,3] out or NULL (= gradient w.r.t. v_shaped).
 *   dposer_lbs_prepare_joint_lists(h, joint_ptr, joint_vidx, joint_w, stream): SETUP call, once per set of lists (and again
 *   whenever their contents change): re-cuts the lists by vertex chunk for the one-pass skinning-backward kernels and stores the
 *   tables in the handle -- among them the skinning weights of every 256-vertex chunk as a dense 64 x 256 matrix in bf16 hi / lo planes,
 *   laid out as MFMA operand fragments (64 KB per chunk: the joint-transform reduction runs on the matrix pipe).  It synchronises the
 *   stream, copies the lists to the host and allocates -- dposer_lbs_backward itself does none of that; without prepared lists it runs
 *   the (pose, joint)-parallel gather kernel, which is the right kernel below ~320 poses anyway.  dposer_lbs_backward forks onto two
 *   internal streams of the handle for the three product terms of its blend-gradient GEMM and joins them before it returns control
 *   of `stream` (events only, no host synchronisation): one call at a time per handle.
 *   dposer_body_tuning_reload(): re-reads the A/B environment switches of the body-model kernels (DPOSER_FK_SMALL_MAX,
 *   DPOSER_LBS_JOINT_STREAM_MIN, DPOSER_LBS_BLEND); they are otherwise read once per process, not per call. */
int dposer_lbs_prepare_joint_lists(dposer_body_t h, const int32_t* joint_ptr, const int32_t* joint_vidx, const float* joint_w, void* stream);
void dposer_body_tuning_reload(void);
int64_t dposer_lbs_posedirs_bwd_packed_bytes(dposer_body_t h);
int dposer_lbs_pack_posedirs_bwd(dposer_body_t h, const float* posedirs, void* packed, void* stream);
/* dposer_lbs_backward_fold: dposer_lbs_backward + the backward of the joint rows that are functions of VERTICES -- smplx
 *   VertexJointSelector (row J + e = vertex extra_vertex_ids[e]) and vertices2landmarks (row J + n_extra + l = barycentric combination of
 *   the three vertices of landmark l; called from lib/body_model/body_model.py:75-88 through smplx.SMPLX.forward): their gradients
 *   d_joints[:, J:] are added to the gradient of the vertices they read.  `fold` (device tables, built once per asset by the caller):
 *     vertex_slot [V]   slot u of the vertex, or -1;      slot_vertex [n_slots]   the vertex of slot u;
 *     slot_ptr [n_slots + 1], entry_row [n], entry_weight [n]: slot u receives sum_e entry_weight[e] * d_joints[:, entry_row[e]] over
 *     e in [slot_ptr[u], slot_ptr[u + 1]), added in that order (deterministic).
 *   d_verts is only READ (the corrected rows live in ws_bwd); fold == NULL is dposer_lbs_backward. */
typedef struct dposer_lbs_joint_fold {
    const int32_t* vertex_slot;
    const int32_t* slot_vertex;
    const int32_t* slot_ptr;
    const int32_t* entry_row;
    const float* entry_weight;
    int32_t n_slots;
} dposer_lbs_joint_fold;
int dposer_lbs_backward_fold(dposer_body_t h, const void* ws_fwd, void* ws_bwd, const void* posedirs_bwd_packed,
                             const float* const* pose_segments_host, const int32_t* segment_joints_host, int32_t num_segments,
                             const float* j_rest, int32_t j_rest_batched, const float* v_shaped, int32_t v_shaped_batched,
                             const int32_t* skin_idx, const float* skin_w, int32_t skin_k, const int32_t* joint_ptr,
                             const int32_t* joint_vidx, const float* joint_w, const float* d_verts, const float* d_joints,
                             int64_t d_joints_ld, const dposer_lbs_joint_fold* fold, float* const* d_pose_segments_host, float* d_jrest,
                             float* d_vposed, int64_t batch, void* stream);
int64_t dposer_lbs_backward_workspace_bytes(dposer_body_t h, int64_t batch);
int dposer_lbs_backward(dposer_body_t h, const void* ws_fwd, void* ws_bwd, const void* posedirs_bwd_packed,
                        const float* const* pose_segments_host, const int32_t* segment_joints_host, int32_t num_segments,
                        const float* j_rest, int32_t j_rest_batched, const float* v_shaped, int32_t v_shaped_batched,
                        const int32_t* skin_idx, const float* skin_w, int32_t skin_k, const int32_t* joint_ptr,
                        const int32_t* joint_vidx, const float* joint_w, const float* d_verts, const float* d_joints,
                        int64_t d_joints_ld, float* const* d_pose_segments_host, float* d_jrest, float* d_vposed,
                        int64_t batch, void* stream);

/* MotionDenoise.optimize -- run/motion_denoising.py:199-300 (DPoser_loss :124-143, weights :157-163, temporal / data terms
 * :253-263): `n_steps` torch.optim.Adam steps on the axis-angle body pose [frames, body joints * 3] of ONE sequence under
 *   w_temp[i] * mean ||v[t] - v[t+1]|| + w_data[i] * mean ||Jtr[:, :n_obs_joints] - joints_obs|| + w_prior[i] * DPoser_loss(normalise(pose)),
 * all steps queued from one call (prior evaluation = dposer_prior_loss, body model = dposer_lbs_forward / _backward, the
 * loss gradients and the Adam update are kernels of this entry).  The data term is dropped for a step when its value is not
 * finite and > 0 (:261-263) -- decided on the device, per sequence: one NaN among a sequence's observed joints drops that
 * sequence's whole term for the step (and logs it as 0), as the reference's guard does; the other sequences are unaffected.
 *   score network: handle, parameters, packed weights, a DPOSER_WS_SHARED_T workspace for `frames` samples and n_steps table rows;
 *   body model: handle + the device tables dposer_lbs_forward / dposer_lbs_backward take, their two workspaces for `frames`
 *   poses; rest_batched: v_shaped / j_rest are [frames, ...] instead of shared; pose segments other than `body_segment` are
 *   the zero pose;  joint_rows = J + num_extra + num_landmarks (row count of the LBS joint output);
 *   norm_mode 0 none / 1 z-score (norm_a = mean, norm_b = std) / 2 min-max (norm_a = min, norm_b = max), arrays [pose dim];
 *   t_host / w_temp_host / w_data_host / w_prior_host [n_steps]: HOST arrays; weighted: the `weighted` flag of DPoser_loss
 *   (False in the reference, :124); adam_m / adam_v zero on entry for a fresh optimiser, adam_step0 = steps already taken;
 *   noise [n_steps, frames, pose dim] injected z of the prior or NULL -> Philox(seed, step0 + i);
 *   scratch: dposer_motion_denoise_scratch_bytes(frames, pose dim, V, joint_rows) bytes, 256-byte aligned;
 *   frames_per_sequence: 0 = one sequence of `frames` frames; F = a batch of frames / F sequences of F consecutive frames each
 *   (independent problems advanced together: temporal neighbours, the data-term decision and the loss means are per sequence; the
 *   in-kernel prior noise is keyed by the frame index inside the batch);
 *   loss_log: DEVICE [n_steps, sequences, 3] (temp, data values of each sequence; the prior value is the batch total, i.e. the sum
 *   over the sequences' prior terms) of every step, unweighted, or NULL.
 *
 * PARTIAL OBSERVATIONS (joints_conf and / or obs_rows, the last two fields; both NULL = everything above, kernel for kernel and bit
 * for bit).  For one sequence of F frames, with observed columns j = 0 .. n_obs_joints - 1 of joints_obs [frames, n_obs_joints, 3]:
 *   rows[j] = obs_rows[j] is the tree joint column j observes (obs_rows == NULL: rows[j] = j).  The entries are distinct and lie in
 *     [0, num_joints) -- tree joints only: dposer_lbs_backward_temporal ignores gradient rows >= num_joints.  (The caller checks this;
 *     the kernel never dereferences a row outside that range -- its column counts as not live.)
 *   c = joints_conf[t, j], float32 [frames, n_obs_joints] (joints_conf == NULL: c = 1).
 *   An entry (t, j) is LIVE iff c > 0 -- false for 0, for negatives and for NaN.
 *   For an entry that is not live, joints_obs[t, j] never enters any sum and may be NaN or Inf; its gradient row is written as 0.
 *   r = J[t, rows[j]] - joints_obs[t, j],  s2 = |r|^2.
 *   W = sum_live c,  N = sum_live c * sqrt(s2 < 1e-36 ? 1e-36 : s2)  (a NaN s2 is not clamped),  data = N / W.
 *   The term is KEPT iff W > 0 and data is finite and data > 0.
 *   d data / d J[t, rows[j]] = w_data * (c / W) * r / sqrt(s2) for the live entries of a kept term with s2 > 1e-36, else 0.
 *   loss_log column 1 holds data when kept and 0 when dropped.
 * Consequences: a sequence with NO live entry (W = 0) keeps moving under the prior and the temporal term alone; a NaN observation under a
 * POSITIVE confidence makes N NaN and drops that sequence's term for the step, exactly as without confidences.  W, N and the decision are
 * per sequence; the sums are fp32 block sums in a fixed order (no atomics), so a call is reproducible bit for bit. */
typedef struct dposer_motion_denoise_args {
    dposer_scorefc_t net;
    const float* flat_params;
    const void* packed;
    void* net_ws;
    const dposer_sde_desc* sde;
    const float* freq;
    const float* sigmas;
    dposer_body_t body;
    void* lbs_ws_fwd;
    void* lbs_ws_bwd;
    const void* posedirs_packed;
    const void* posedirs_bwd_packed;
    const float* j_rest;
    const float* v_shaped;
    int32_t rest_batched;
    const int32_t* skin_idx;
    const float* skin_w;
    int32_t skin_k;
    const int32_t* joint_ptr;
    const int32_t* joint_vidx;
    const float* joint_w;
    const int32_t* extra_vertex_ids;
    const int32_t* lmk_tri;
    const float* lmk_bary;
    const int32_t* segment_joints_host;
    int32_t num_segments;
    int32_t body_segment;
    int32_t num_vertices;
    int32_t num_joints;
    int32_t joint_rows;
    int64_t frames;       /* sequences x frames_per_sequence, at most 65535 per call (sequences are independent: a larger batch goes through in groups
                             of whole sequences, as MotionDenoise.optimize_sequences does) */
    int64_t frames_per_sequence;
    float* pose;
    float* adam_m;
    float* adam_v;
    const float* joints_obs;
    int32_t n_obs_joints;
    int32_t norm_mode;
    const float* norm_a;
    const float* norm_b;
    int32_t n_steps;
    int32_t weighted;
    const float* t_host;
    const float* w_temp_host;
    const float* w_data_host;
    const float* w_prior_host;
    double lr, beta1, beta2, eps;
    int32_t adam_step0;
    uint32_t step0;
    uint64_t seed;
    const float* noise;
    void* scratch;
    float* loss_log;
    int32_t rot6d;        /* != 0: the score network works on the 6-D rotation representation (rot_rep = 'rot6d': 6 J inputs, norm_a / norm_b
                             hold 6 J statistics, noise is [n_steps, frames, 6 J]); the pose being optimised stays axis-angle */
    const float* joints_conf;     /* DEVICE [frames, n_obs_joints] confidences of PARTIAL OBSERVATIONS above, or NULL = 1 everywhere */
    const int32_t* obs_rows;      /* DEVICE [n_obs_joints] distinct tree joints in [0, num_joints) the columns observe, or NULL = 0 .. n_obs_joints - 1 */
} dposer_motion_denoise_args;
int64_t dposer_motion_denoise_scratch_bytes(int64_t frames, int32_t pose_dim, int32_t num_vertices, int32_t joint_rows);
int dposer_motion_denoise_optimize(const dposer_motion_denoise_args* args, void* stream);

/* SMPLify -- run/smplify.py:118-281 (SMPLify.__call__; losses lib/body_model/fitting_losses.py:57-131): B independent fits of SMPL-X to
 * 2D keypoints, all num_iters + n_stages * num_iters torch.optim.Adam iterations queued from one call:
 *   camera stage (:200-222): Adam over [global_orient | cam_t] on camera_fitting_loss (sum over the batch: OP hips / shoulders, or the
 *     four GT joints for an image whose OP confidences are not all > 0, plus depth_weight^2 (t_z - t_z_est)^2);
 *   confidences of ign_joints zeroed in `keypoints` (:238);
 *   body stage (:240-263): a fresh Adam over [body_pose | betas | global_orient] on body_fitting_loss (mean over the batch: GMoF reprojection
 *     with conf^2, w_pose^2 * DPoser prior (sum / batch_size at the iteration's t, weight 0.5 sqrt(1 + SNR)), w_angle^2 * angle prior,
 *     w_shape^2 * |betas|^2) with the weights of stage s = k / num_iters (:145-149);
 *   reprojection [B, n_keypoints] out: conf^2 * GMoF of the final parameters (:266-277).
 * The camera translation reaches the projection only as transl of the body model (fitting_losses.py:8-38 never reads its translation).
 * Body model: a handle whose mesh is just the vertices the mapped extra joints read (rows [num_joints, joint_rows) of the LBS joint output,
 * vertex-selected through extra_vertex_ids, no landmarks); v_template / shapedirs [V, 3, num_shape] of those vertices, j_template / jdirs of
 * the full asset; shape [B, num_shape]: the first num_betas columns are the betas being fitted, the rest stay as given (expression).
 *   joint_map [n_keypoints]: LBS joint row of each keypoint; map_ptr [joint_rows + 1] / map_entry: keypoints of each row (their gradients are
 *   summed in that order -- no atomics);  op_joints / gt_joints: keypoint indices of camera_fitting_loss (:97-100).
 *   batch images of a larger problem of inv_batch = 1 / B_global images starting at global image row0: the prior noise is keyed by the
 *   global image index (Philox(seed, step0 + k) when noise == NULL, else noise [n_stages * num_iters, batch, network inputs]).
 *   t_host [n_stages * num_iters]; w_pose_host / w_shape_host / w_angle_host [n_stages]: HOST arrays.
 *   scratch: dposer_smplify_scratch_bytes(batch, V, J, joint_rows, num_shape, network inputs) bytes, 256-byte aligned.
 *   loss_log: DEVICE [num_iters * (1 + n_stages), batch, 4] or NULL: camera rows (camera loss, 0, 0, depth term), body rows (reprojection,
 *   angle, shape, prior) weighted as they enter the loss.  Columns 0-2 (and the camera rows) are per image and do not depend on how a
 *   larger problem is split into calls.  The prior entry is the one per-call quantity: w_pose^2 * inv_batch * (sum over THIS call's
 *   `batch` images), the same value in every image's row -- one call over the whole problem logs the loss's sum / batch_size term, and the
 *   entries of the calls a problem is split into add up to it.
 * Allocates nothing, never synchronises the host. */
typedef struct dposer_smplify_args {
    dposer_scorefc_t net;
    const float* flat_params;
    const void* packed;
    void* net_ws;
    const dposer_sde_desc* sde;
    const float* freq;
    const float* sigmas;
    dposer_body_t body;
    void* lbs_ws_fwd;
    void* lbs_ws_bwd;
    const void* posedirs_packed;
    const void* posedirs_bwd_packed;
    const float* v_template;
    const float* shapedirs;
    const float* j_template;
    const float* jdirs;
    const int32_t* skin_idx;
    const float* skin_w;
    int32_t skin_k;
    const int32_t* joint_ptr;
    const int32_t* joint_vidx;
    const float* joint_w;
    const int32_t* extra_vertex_ids;
    const dposer_lbs_joint_fold* fold;
    const int32_t* segment_joints_host;
    int32_t num_segments;
    int32_t orient_segment;
    int32_t body_segment;
    int32_t num_vertices;
    int32_t num_joints;
    int32_t joint_rows;
    int32_t num_shape;
    int32_t num_betas;
    int64_t batch;        /* at most 65535 images per call (one grid row per pose in the skinning kernels) */
    int64_t row0;
    float inv_batch;
    int32_t n_keypoints;  /* <= 64: one wave per image */
    const int32_t* joint_map;
    const int32_t* map_ptr;
    const int32_t* map_entry;
    int32_t op_joints[4];
    int32_t gt_joints[4];
    int32_t ign_joints[8];
    int32_t n_ign;
    float* keypoints;             /* [B, n_keypoints, 3] (x, y, confidence) */
    const float* focal_length;    /* [B] */
    const float* camera_center;   /* [B, 2] */
    const float* cam_t_est;       /* [B, 3] */
    float* global_orient;         /* [B, 3] */
    float* body_pose;             /* [B, body joints * 3] */
    float* shape;                 /* [B, num_shape] */
    float* cam_t;                 /* [B, 3] */
    int32_t norm_mode;
    const float* norm_a;
    const float* norm_b;
    int32_t rot6d;
    int32_t num_iters;
    int32_t n_stages;
    const float* t_host;
    const float* w_pose_host;
    const float* w_shape_host;
    const float* w_angle_host;
    float sigma;
    float depth_weight;
    double lr, beta1, beta2, eps;
    uint64_t seed;
    uint32_t step0;
    const float* noise;
    void* scratch;
    float* loss_log;
    float* reprojection;          /* [B, n_keypoints] */
} dposer_smplify_args;
int64_t dposer_smplify_scratch_bytes(int64_t batch, int32_t num_vertices, int32_t num_joints, int32_t joint_rows, int32_t num_shape,
                                     int32_t net_inputs);
int dposer_smplify_optimize(const dposer_smplify_args* args, void* stream);

/* Mesh self-intersections -- the SI metric of run/demo.py:148-161 (lib/utils/metric.py:41-92 delegates to PyMeshLab's
 * compute_selection_by_self_intersections_per_face): for B meshes sharing one face list, which faces intersect another face of their mesh.
 * Pair rule, from the vertex INDICES of faces f != g (a face with a repeated index is degenerate: never tested, never flagged):
 *   3 shared indices (duplicate face): intersect;  2 (an edge): do not;
 *   1 shared vertex s: with a, b f's other two vertices, the segment (s+a)/2 -> (s+b)/2 crosses g at a point strictly inside g (barycentric
 *     (b1, b2) on g's 2nd / 3rd vertex: b1 > 1e-6, b2 > 1e-6, b1 + b2 < 1; the segment's ends count), or the same with f and g swapped;
 *   0 shared: Moller's triangle-triangle test with its coplanar branch, touching counts as intersecting.
 * Pairs whose bounding boxes do not meet (closed boxes) are not tested.  The 0-shared test runs with the pair in a fixed order (sorted vertex
 * indices, lexicographic), so the flags do not depend on the order of the faces, the tiling or the schedule.  All arithmetic fp32.
 *   vertices [batch, num_vertices, 3];  faces [num_faces, 3] int32, indices in [0, num_vertices) (not checked: device data);
 *   face_order [num_faces]: a permutation of the faces that makes runs of 64 consecutive faces compact surface patches (only the speed of the
 *     tile culling depends on it), or NULL for the identity;
 *   flags [batch, num_faces] out: 1 where the face intersects another face of its mesh, else 0;  counts [batch] out: flagged faces per mesh;
 *   scratch: dposer_mesh_self_intersections_scratch_bytes(batch, num_faces) bytes, 256-byte aligned.
 * DPOSER_SI_ALLPAIRS=1 (read once per process, dposer_body_tuning_reload re-reads it): every tile pair is walked, no tile culling -- the
 * cross-check that culling changes no flag.  Allocates nothing, never synchronises the host. */
typedef struct dposer_mesh_si_args {
    const float* vertices;
    int64_t batch;
    int32_t num_vertices;
    const int32_t* faces;
    int32_t num_faces;
    const int32_t* face_order;
    uint8_t* flags;
    int32_t* counts;
    void* scratch;
} dposer_mesh_si_args;
int64_t dposer_mesh_self_intersections_scratch_bytes(int64_t batch, int32_t num_faces);
int dposer_mesh_self_intersections(const dposer_mesh_si_args* args, void* stream);

/* Batched mesh rendering -- what lib/body_model/visual.py:132-366 does with pyrender / pytorch3d (render_mesh, multiple_render,
 * faster_render, Renderer): B meshes sharing one face list, rasterised with a depth test into num_images images in one call.
 * Frames: vertices are in the model frame; transforms [B, 3, 4] (row-major) take them to the camera frame, OpenCV's (x right, y down,
 * z forward); image n projects u = fx x / z + cx, v = fy y / z + cy with intrinsics[n] = (fx, fy, cx, cy).  Pixel (row i, col j) covers
 * [j, j+1) x [i, i+1) and is sampled at its centre (j + 0.5, i + 0.5).  Mesh b is drawn into image image_of_mesh[b] (NULL: image b);
 * meshes of one image are depth-tested together.  Each vertex is projected exactly once per mesh.
 * Coverage: with the projected corners of a face in its index order, each edge function is evaluated in fp32 with its endpoints in
 *   canonical order (lower vertex index first: E = (x_hi - x_lo)(py - y_lo) - (y_hi - y_lo)(px - x_lo)) and negated as the face's winding
 *   and the sign of its area require, so that the interior is positive.  A centre is covered when every edge value is > 0, or == 0 on an
 *   edge that is top-left in that orientation (direction (dx, dy) with dy < 0, or dy == 0 and dx > 0).  Either winding, no culling.  Two
 *   faces that share an edge see exactly opposite values on it, so no centre on a shared edge is missed or covered twice.
 * Depth: perspective-correct, z = 1 / sum_i b_i / z_i with b_i the edge values normalised by their sum.  The key of a fragment is
 *   (bits of z) << 32 | (b * num_faces + f) and the smallest key wins: the nearest fragment, ties to the lower (mesh, face), whatever the
 *   launch order, face order or grouping.  b * num_faces + f must stay below 2^32 - 1 (checked).
 * Dropped faces (never write anything): a corner with z <= znear (no clipping, unlike OpenGL), all corners beyond zfar (a face that
 *   straddles zfar is drawn whole), zero area in fp32, a non-finite corner, a repeated vertex index.
 * Shading: c = clamp(base * (ambient + sum_l I_l max(0, n . l)), 0, 1), 8-bit value rint(255 c), no specular term.  l is the unit vector
 *   toward the light: lights[l] = (kind, x, y, z, r, g, b), kind 0 = directional (x, y, z: direction toward the light), 1 = point
 *   (position; no attenuation), all in the camera frame.  n is the camera-frame face normal (smooth = 0), or (smooth = 1) the
 *   perspective-correct interpolation of vertex normals, each the normalised sum of the unit normals of the faces around it (a
 *   vertex -> face CSR built on the host, vf_ptr [V + 1] / vf_face; render_meshes orders a vertex's faces by their sorted vertex
 *   indices, so the sum does not depend on the face order); n is turned to face the
 *   camera at the shaded point.  Uncovered pixels take background [H, W, 3] (+ n * background_stride bytes for image n; stride 0:
 *   shared), or background_color when background is NULL.
 * Outputs (each optional, NULL = not written), [num_images, H, W]: rgb uint8 [.., 3]; depth fp32 (camera z, 0 where empty); face_id and
 *   mesh_id int32 (-1 where empty).  scratch: dposer_render_scratch_bytes(...) bytes, 256-byte aligned.  faces / image_of_mesh / vf_* are
 *   device data and not range-checked here.  Allocates nothing, never synchronises the host. */
#define DPOSER_LIGHT_DIRECTIONAL 0
#define DPOSER_LIGHT_POINT 1
typedef struct dposer_render_args {
    const float* vertices;        /* [num_meshes, num_vertices, 3] */
    int64_t num_meshes;
    int32_t num_vertices;
    const int32_t* faces;         /* [num_faces, 3] */
    int32_t num_faces;
    const float* transforms;      /* [num_meshes, 3, 4] */
    const int32_t* image_of_mesh; /* [num_meshes] or NULL */
    int64_t num_images;
    int32_t height, width;
    const float* intrinsics;      /* [num_images, 4] */
    float znear, zfar;
    const float* base_color;      /* [num_meshes, 3] */
    const float* lights;          /* [num_lights, 7] */
    int32_t num_lights;
    float ambient[3];
    int32_t smooth;
    const int32_t* vf_ptr;        /* [num_vertices + 1], smooth only */
    const int32_t* vf_face;       /* [vf_ptr[num_vertices]], smooth only */
    const uint8_t* background;    /* [H, W, 3] or NULL */
    int64_t background_stride;    /* bytes between the backgrounds of consecutive images; 0 = one shared */
    uint8_t background_color[4];  /* RGB (+ pad) where background is NULL */
    uint8_t* rgb;
    float* depth;
    int32_t* face_id;
    int32_t* mesh_id;
    void* scratch;
} dposer_render_args;
int64_t dposer_render_scratch_bytes(int64_t num_meshes, int32_t num_vertices, int32_t num_faces, int64_t num_images, int32_t height,
                                    int32_t width);
int dposer_render_meshes(const dposer_render_args* args, void* stream);

/* Rigid (similarity) alignment -- lib/utils/transforms.py:264-286 (rigid_transform_3D, rigid_align) for B independent pairs of point sets
 * src = A, dst = B, each [batch, num_points, 3] fp32, num_points >= 1.  Per pair:
 *   centroids a, b;  H = (A - a)^T (B - b) / N;  H = U S V^T;  R = V U^T;  if det R < 0 the last singular value and the last row of V^T
 *   are negated and R re-formed, so R is always a proper rotation;  c = sum(s) / sum over axes of the population variance of A
 *   (np.var, ddof 0);  t = b - c R a.
 * Outputs, each optional (NULL = not written): transform [batch, 13] = (c, R row-major, t); aligned [batch, num_points, 3] = c R a + t;
 *   mean_dist [batch] = mean over points of ||aligned - dst||_2, in the caller's unit.
 * Arithmetic: centroids, H, the variance, the 3 x 3 decomposition (one-sided Jacobi, written in the kernel), c, R and t in fp64, from
 *   moments taken relative to the pair's first point; the transform is rounded once to fp32, and c R a + t and the distances are fp32
 *   FMAs on the rounded transform (distances summed in fp64).  Every sum runs in a fixed order that depends on num_points alone (no
 *   atomics): the bits of a pair do not depend on batch, on its position, or on how a batch is split into calls.
 * A pair whose source has zero variance (num_points = 1 included) or that holds a non-finite coordinate gets NaN in all its outputs, as
 *   the reference's division by zero does; other pairs are unaffected.  Collinear sources are ill-conditioned here as in the reference.
 * Allocates nothing, never synchronises the host. */
typedef struct dposer_rigid_align_args {
    const float* src;         /* [batch, num_points, 3] */
    const float* dst;         /* [batch, num_points, 3] */
    int64_t batch;
    int32_t num_points;
    float* transform;         /* [batch, 13] or NULL */
    float* aligned;           /* [batch, num_points, 3] or NULL */
    float* mean_dist;         /* [batch] or NULL */
} dposer_rigid_align_args;
int dposer_rigid_align(const dposer_rigid_align_args* args, void* stream);

/* Joint regression -- np.dot(J_regressor, mesh)[:R] of lib/dataset/mocap_dataset.py:72-73 for B meshes: joints [batch, num_rows, 3] =
 * W vertices [batch, num_vertices, 3] with W in CSR form (row_ptr [num_rows + 1], col, weight; the host builds it once per model).  A
 * row's entries are summed in CSR order in fp64 and rounded once to fp32; only the vertices a row names are read.  The weights are
 * fp32: a regressor stored in fp64 is rounded once per weight before the sums (up to 6e-8 relative on a joint, 2e-7 m at 4 m; the
 * regressors of the SMPL-family files the loader reads are kept in fp32 by the body model as well).  col is device data and not
 * range-checked here.  Allocates nothing, never synchronises the host. */
typedef struct dposer_regress_joints_args {
    const float* vertices;
    int64_t batch;
    int32_t num_vertices;
    const int32_t* row_ptr;
    const int32_t* col;
    const float* weight;
    int32_t num_rows;
    float* joints;
} dposer_regress_joints_args;
int dposer_regress_joints(const dposer_regress_joints_args* args, void* stream);

/* EHF evaluation -- MocapDataset.eval_EHF (lib/dataset/mocap_dataset.py:61-84) for B images in one call.  Both meshes are regressed to
 * num_rows joints (the rule of dposer_regress_joints); the ground-truth joints are rotated by gt_rotation (row-major 3 x 3, applied to the
 * fp64 sums before rounding; NULL = identity; the reference rotates the whole mesh first, which is the same up to rounding because the
 * regressor is linear); the predicted joints are aligned onto them (the rule of dposer_rigid_align);
 *   pa_mpjpe = 1000 mean_j ||aligned_j - gt_j||;   mpjpe = 1000 mean_j ||pred_j - pred_pelvis + gt_pelvis - gt_j||  (pelvis = pelvis_row).
 * pred_joints, gt_joints, aligned_joints [batch, num_rows, 3] are optional outputs.  scratch: dposer_ehf_eval_scratch_bytes(batch,
 * num_rows) bytes, 256-byte aligned.  Queues its kernels on the stream; allocates nothing, never synchronises the host. */
typedef struct dposer_ehf_eval_args {
    const float* pred_vertices;   /* [batch, num_vertices, 3] */
    const float* gt_vertices;     /* [batch, num_vertices, 3] */
    int64_t batch;
    int32_t num_vertices;
    const int32_t* row_ptr;
    const int32_t* col;
    const float* weight;
    int32_t num_rows;
    const float* gt_rotation;     /* [3, 3] or NULL */
    int32_t pelvis_row;
    float* pa_mpjpe;              /* [batch], millimetres when the meshes are in metres */
    float* mpjpe;                 /* [batch] */
    float* pred_joints;
    float* gt_joints;
    float* aligned_joints;
    void* scratch;
} dposer_ehf_eval_args;
int64_t dposer_ehf_eval_scratch_bytes(int64_t batch, int32_t num_rows);
int dposer_ehf_eval(const dposer_ehf_eval_args* args, void* stream);

/* Skeleton plots -- what lib/body_model/visual.py:18-119 does with one matplotlib 3-D figure per frame (visualize_3d_skeleton,
 * visualize_skeleton_sequence, vis_skeletons): B frames of J joints drawn as K bones and J discs in one call, every frame under the same
 * orthographic view.  Pixel (row y, col x) is sampled at its centre (x + 0.5, y + 0.5).  All arithmetic fp32, no contraction.
 * Projection: screen x = cx + s (X - X0);  screen y = cy - s (Y - Y0) when y_up = 1, cy + s (Y - Y0) when y_up = 0;  depth = -Z when
 *   z_toward_viewer = 1 (larger Z is nearer), else Z.  A larger depth is farther.  y_up = 1, z_toward_viewer = 1 is the reference's view
 *   (vis_skeletons flips the points by pi about x, then plots (x, z, -y) at view_init(0, -90): an upright front view of the input joints).
 * Primitives: K bones, the screen-space segments between joints bones[k][0] and bones[k][1]; a bone is dropped when either end is
 *   invisible (visible[j] == 0; visible NULL = all visible) or has a non-finite coordinate.  Then J discs at the joints, dropped on the
 *   same conditions.  Primitive index: bone k -> k, disc j -> K + j.
 * Coverage at a pixel centre: a = clamp(r + 0.5 - d, 0, 1); bone: d = distance to the segment (the nearest point a + t (b - a), t =
 *   clamp((p - a) . (b - a) / |b - a|^2, 0, 1), t = 0 for a zero-length segment), r = line_width / 2; disc: d = distance to the centre,
 *   r = joint_radius.
 * Order: painter's, per frame.  One key per primitive: a bone's is 0.5 (depth_a + depth_b), a disc's its joint's depth - 1e-3 (a disc
 *   lies in front of the bones that meet at it).  Painted far to near (descending key), ties in primitive index order (mplot3d orders
 *   its artists the same way, one depth per artist).
 * Colour: c starts as the background pixel (background [H, W, 3] + b * background_stride bytes for frame b, stride 0: shared; or
 *   background_color when background is NULL); for each primitive in order with a > 0, c <- c (1 - a) + colour a per channel; the stored
 *   byte is rint(c).
 * Limits: num_bones + num_joints <= DPOSER_DRAW_MAX_PRIMITIVES; batch x tiles must fit 31 bits.  bones is device data and not
 *   range-checked here.  scratch: dposer_draw_skeletons_scratch_bytes(batch, num_joints, num_bones) bytes, 256-byte aligned.  Addresses
 *   are 64-bit throughout (batch x H x W x 3 may pass 2^31).  No atomics; allocates nothing, never synchronises the host. */
#define DPOSER_DRAW_MAX_PRIMITIVES 4096
typedef struct dposer_draw_skeletons_args {
    const float* joints;          /* [batch, num_joints, 3] */
    int64_t batch;
    int32_t num_joints;
    int32_t num_bones;
    const uint8_t* visible;       /* [num_joints] or NULL */
    const int32_t* bones;         /* [num_bones, 2] */
    const uint8_t* bone_color;    /* [num_bones, 3] RGB */
    const uint8_t* joint_color;   /* [num_joints, 3] RGB */
    float s, X0, Y0, cx, cy;
    int32_t y_up, z_toward_viewer;
    float line_width, joint_radius;
    int32_t height, width;
    const uint8_t* background;    /* [H, W, 3] or NULL */
    int64_t background_stride;    /* bytes between the backgrounds of consecutive frames; 0 = one shared */
    uint8_t background_color[4];  /* RGB (+ pad) where background is NULL */
    uint8_t* rgb;                 /* [batch, H, W, 3] */
    void* scratch;
} dposer_draw_skeletons_args;
int64_t dposer_draw_skeletons_scratch_bytes(int64_t batch, int32_t num_joints, int32_t num_bones);
int dposer_draw_skeletons(const dposer_draw_skeletons_args* args, void* stream);

/* Panel compositor -- what lib/utils/motion_video.py:6-55,95-126 does per frame with numpy and cv2 (crop_bottom, cv2.resize,
 * resize_or_crop, add_title, np.hstack): N output frames [N, out_h, out_w, 3] from num_panels panels each, in one call.  Panel p owns the
 * output columns [x_offset, x_offset + cell_w) and rows [0, cell_h + strip_h); a later panel overwrites an earlier one where they overlap;
 * pixels no panel owns take out_fill.  Inside its cell (rows < cell_h), for frame n:
 *   source  S = src + n * src_stride bytes, uint8 [src_h, src_w, 3] (stride 0: one image shared by every frame);
 *   crop    C[i][j] = S[crop_y + i][crop_x + j], i < crop_h, j < crop_w;
 *   resize  R = C when (resize_h, resize_w) == (crop_h, crop_w) (exact byte move).  Otherwise bilinear with cv2.INTER_LINEAR's documented
 *           geometry, per axis: u = (dst + 0.5) * (crop / resize) - 0.5, i0 = floor(u), f = u - i0, taps i0 and i0 + 1 clamped to
 *           [0, crop - 1]; value = (1 - fy) ((1 - fx) p00 + fx p01) + fy ((1 - fx) p10 + fx p11) in fp32 (no contraction), stored as rint.
 *           (cv2's fixed-point path is not reproduced.)
 *   place   resize_or_crop(R, cell_w, cell_h), each axis on its own: a wider R keeps its centre columns (left = (resize_w - cell_w) / 2), a
 *           narrower one is centred over fill (left = (cell_w - resize_w) / 2); a taller R keeps its bottom rows, a shorter one is
 *           bottom-aligned over fill.  (The reference's narrow-and-wrong-height case raises a numpy shape error; here it is defined.)
 * Rows cell_h <= y < cell_h + strip_h take strip [strip_h, cell_w, 3] (NULL: strip_h must be 0).  At most DPOSER_MAX_PANELS panels.
 * Every crop must lie inside its source (checked).  Allocates nothing, never synchronises the host. */
#define DPOSER_MAX_PANELS 8
typedef struct dposer_panel {
    const uint8_t* src;           /* [N or 1, src_h, src_w, 3] */
    int64_t src_stride;           /* bytes between the sources of consecutive frames; 0 = one shared */
    int32_t src_h, src_w;
    int32_t crop_x, crop_y, crop_w, crop_h;
    int32_t resize_h, resize_w;
    int32_t cell_h, cell_w;
    uint8_t fill[4];              /* RGB (+ pad) */
    const uint8_t* strip;         /* [strip_h, cell_w, 3] or NULL */
    int32_t strip_h;
    int32_t x_offset;
} dposer_panel;
typedef struct dposer_compose_args {
    const dposer_panel* panels;   /* host array [num_panels] */
    int32_t num_panels;
    int64_t num_frames;
    int32_t out_h, out_w;
    uint8_t out_fill[4];          /* RGB (+ pad) */
    uint8_t* out;                 /* [num_frames, out_h, out_w, 3] */
} dposer_compose_args;
int dposer_compose_panels(const dposer_compose_args* args, void* stream);

/* Shuffled mini-batch gather -- the data feed of the training loop (run/train.py:70-93: a shuffling DataLoader with drop_last over a dataset
 * of single poses), stateless and on the device: row r of the outputs is dataset row pi(seed, epoch, base + r), r in [0, B).
 * Permutation rule.  pi(seed, epoch, .) is a bijection of [0, N), evaluated per row in the kernel; nothing is stored or sorted.  It is part
 * of the ABI: the step -> rows map of a training run, and so what a resumed checkpoint trains on next, depends on it.
 *   bits = ceil(log2 N) (0 for N = 1);  k = max(2, 2 ceil(bits / 2));  h = k / 2;  mask = 2^h - 1      (2^k < 4 N; N <= 2^62, so h <= 31)
 *   x = p;  repeat
 *       L = x >> h;  R = x & mask
 *       for round = 0, 1, 2, 3:   F = philox4x32-10(counter = (R, epoch, 8, round), key = (seed & 0xffffffff, seed >> 32)) word 0, & mask
 *                                 (L, R) = (R, L ^ F)
 *       x = L << h | R
 *   until x < N;  pi(seed, epoch, p) = x
 *   (a balanced 4-round Feistel network on k bits, cycle-walked into [0, N): a bijection of [0, 2^k) restricted to the values below N, under
 *   4 evaluations expected.  8 is the Philox stream id of the feed, distinct from every stream of the score and sampler kernels.)
 *   data [N, D] fp32 row-major, any D >= 1 (rows are assumed 4-byte aligned only);  aux [N_aux >= N, D_aux] fp32 or NULL, gathered with the
 *   same row index (the dataset's shapes, which the reference indexes un-subsampled with the pose index, lib/dataset/AMASS.py:56-58);
 *   out [B, D], aux_out [B, D_aux], indices [B] int64 (the row indices themselves): each may be NULL, at least one is not; out needs data,
 *   aux_out needs aux.  base >= 0, base + B <= N.  Offsets are 64-bit throughout (N D may pass 2^31 elements).
 * One launch.  Allocates nothing, never synchronises the host. */
typedef struct dposer_batch_gather_args {
    const float* data;
    int64_t N;
    int32_t D;
    const float* aux;
    int64_t N_aux;
    int32_t D_aux;
    int64_t base;
    int64_t B;
    uint64_t seed;
    uint32_t epoch;
    float* out;
    float* aux_out;
    int64_t* indices;
} dposer_batch_gather_args;
int dposer_batch_gather(const dposer_batch_gather_args* args, void* stream);

/* All-pairs pose-set distances -- the sum, the k nearest references of every row and the count of references whose radius covers a row, over
 * the matrix d(a_i, b_j) of two pose sets A [na, J, 3] and B [nb, J, 3] (fp32, contiguous), in one call and without storing the matrix.  APD,
 * the nearest-neighbour distance to a reference set and the k-NN manifold scores (precision / recall, density / coverage) all reduce over it.
 * Distance.  d(a, b) = (1 / J) sum_j ||a_j - b_j||, the distance of lib/utils/metric.py:8-37.  The differences are formed directly (never
 *   |a|^2 + |b|^2 - 2 a.b, which cancels exactly where nearest neighbours live).  Per joint: dx = ax - bx, dy, dz; s = fma(dz, dz, fma(dy, dy,
 *   dx dx)); one v_sqrt_f32 (1 ulp).  The joints are added in index order in fp32, starting from 0, then one multiply by the fp32 value of 1 / J.
 *   A distance is a function of the two poses and J alone: not of k, the outputs asked for, the split or the pose's position in its set.
 * Self exclusion.  same_set != 0: B is A (b = a or NULL, nb = na); column j == i is left out of the k-NN and covered outputs of row i.  Only
 *   the index is excluded: another row equal to a_i is its neighbour at distance 0.
 * Outputs, any subset (NULL = not wanted, at least one is wanted):
 *   sum      double[1]: sum_i sum_j d(a_i, b_j), the diagonal of the same set included -- it is exactly 0, so APD = sum / (n (n - 1)).  A lane
 *            adds the distances of at most 16 consecutive references of a tile in fp32, then in fp64: a row's tiles in order, the 64 rows of
 *            a wave by xor butterfly, the four waves of a workgroup in order, the workgroups' sums (row block major, split minor) by 256
 *            strided sums and the same tree.  With same_set and sum alone the tiles left of a row block's own 256 columns are skipped and the
 *            tiles right of them count twice (d is symmetric bit for bit).  No atomics: the order depends on (na, nb, J, k, splits) and on
 *            which outputs are asked for, and two calls on the same inputs return the same bits.
 *   knn_dist float[na, k], knn_idx int32[na, k], 1 <= k <= 8: the k smallest distances of each row, ascending; equal distances in index
 *            order; fewer than k candidates: the tail is +inf / -1.
 *   covered  int32[na]: the count of j with d(a_i, b_j) <= radii[j]; radii float[nb] is required with it.
 *   NaN: a NaN distance is never a neighbour and never covers; sum propagates it.  (A +inf distance is never a neighbour either.)
 * Limits: 1 <= J <= 128, na >= 1, 1 <= nb < 2^31; na nb may pass 2^32.  Everything else is refused (DPOSER_ERR_BAD_ARG) before a launch.
 * Plan.  Workgroups of plan[0] rows (one lane per row) stream tiles of plan[1] references through LDS; the references are cut into `splits`
 *   ranges of whole tiles across the grid, and a second pass merges the partial k-lists, counts and sums in split order, so no output but the
 *   last bits of sum depends on the split.  plan[2] is the split count the library chooses for splits = 0; splits > 0 forces that many, up to
 *   one per tile and at most 64.  plan[3] = 1: J = 22 rows are kept in registers; 0: the general path (both sets pass through LDS in chunks
 *   of 8 joints).  dposer_pose_set_distances_plan is a pure function of its arguments.
 * scratch: dposer_pose_set_distances_scratch_bytes(na, nb, joints, k, splits) bytes (< 0: refused), 256-byte aligned.  Queues up to three
 *   kernels on the stream; allocates nothing, never synchronises the host.
 * Cost note: a (pair, joint) is 3 v_sub + v_mul + 2 v_fma + v_sqrt_f32 + v_add = 7 x 4 + 8 = 36 issue cycles per wave, so the VALU issue floor
 *   is 256 CUs x 4 SIMDs x 64 lanes / 36 cycles x clock = 3.6e12 pair-joints/s at 2 GHz (measured: profiles/set_dist_time.md).
 * Layout (LP64): pointers and int64 at 8-byte alignment, int32 at 4; sizeof = 104. */
typedef struct dposer_set_dist_args {
    const float* a;                   /*   0: [na, joints, 3] */
    const float* b;                   /*   8: [nb, joints, 3]; same_set: a or NULL */
    int64_t na;                       /*  16 */
    int64_t nb;                       /*  24 */
    int32_t joints;                   /*  32 */
    int32_t same_set;                 /*  36 */
    int32_t k;                        /*  40 */
    const float* radii;               /*  48: [nb] or NULL */
    double* sum;                      /*  56: [1] or NULL */
    float* knn_dist;                  /*  64: [na, k] or NULL */
    int32_t* knn_idx;                 /*  72: [na, k] or NULL */
    int32_t* covered;                 /*  80: [na] or NULL */
    int32_t splits;                   /*  88: 0 = the library chooses */
    void* scratch;                    /*  96 */
} dposer_set_dist_args;
int64_t dposer_pose_set_distances_scratch_bytes(int64_t na, int64_t nb, int32_t joints, int32_t k, int32_t splits);
int dposer_pose_set_distances_plan(int64_t na, int64_t nb, int32_t joints, int32_t k, int32_t plan[4]);
int dposer_pose_set_distances(const dposer_set_dist_args* args, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DPOSER_HIP_H */
