// The joint-residual stage of a 3D-joint measurement operator on a normalised body pose (include/dposer_hip.h has the contract):
//   pose = denormalise(y0);  J = FK(pose) over the 22 body joints;  s = sum_live c |J_rows[j] - o_j|^2;  v = 1/2 d s / d y0.
// and the keypoint-residual stage, the same around a pinhole camera and the robust reprojection residual of SMPLify:
//   (ru, rv) = focal J_xy / J_z - (k - centre);  s = sum_live c^2 (rho(ru) + rho(rv)),  live: c > 0 and J_z > z_near.
// FK forward and its gradient are dposer_fk_joints / the reverse walk of dposer_fk_joints_backward (fk.hip); the kernels here are the three
// small passes around them.  fp32 throughout; every sum is taken by one lane in ascending index order.
#include <hip/hip_runtime.h>

#include "../../include/dposer_hip.h"
#include "common.h"
#include "kernels_api.h"

namespace {
constexpr int JG_D = 63;            // 21 body joints, axis-angle
constexpr int JG_NJ = 22;           // root + body: the joints the stage poses
constexpr int JG_ROW = JG_NJ * 3;

// offline_denormalize (lib/dataset/AMASS.py:139-148): mode 0 identity, 1 z-score (a = mean, b = std), 2 min-max (a = min, b = max)
__global__ void __launch_bounds__(256) k_jg_denorm(const float* __restrict__ y0, int mode, const float* __restrict__ a, const float* __restrict__ b,
                                                   float* __restrict__ pose, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c = (int)(i % JG_D);
    const float y = y0[i];
    float p = y;
    if (mode == 1) p = y * b[c] + a[c];
    else if (mode == 2) p = 0.5f * ((y + 1.0f) * (b[c] - a[c]) + 2.0f * a[c]);
    pose[i] = p;
}

// One lane per pose: the gradient row c r of every live entry (zeros elsewhere) and s = sum_live c |r|^2, columns in ascending order.
// live iff c > 0 (false for 0, negatives and NaN) and the row is a joint the stage poses; a dead entry's observation is never read.
__global__ void __launch_bounds__(64) k_jg_resid(const float* __restrict__ posed, const float* __restrict__ obs, const float* __restrict__ conf,
                                                 const int32_t* __restrict__ rows, int n_obs, float* __restrict__ dj, float* __restrict__ s, int64_t B) {
    const int64_t b = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    float* g = dj + b * JG_ROW;
    for (int k = 0; k < JG_ROW; ++k) g[k] = 0.f;
    const float* P = posed + b * JG_ROW;
    float acc = 0.f;
    for (int j = 0; j < n_obs; ++j) {
        const int row = rows ? rows[j] : j;
        const float c = conf ? conf[b * n_obs + j] : 1.0f;
        if (!(c > 0.f) || row < 0 || row >= JG_NJ) continue;
        const float* o = obs + (b * n_obs + j) * 3;
        const float rx = P[3 * row] - o[0], ry = P[3 * row + 1] - o[1], rz = P[3 * row + 2] - o[2];
        g[3 * row] = c * rx; g[3 * row + 1] = c * ry; g[3 * row + 2] = c * rz;
        acc += c * ((rx * rx + ry * ry) + rz * rz);
    }
    s[b] = acc;
}

// One lane per pose: 1/2 d s / d posed joint of every live entry (zeros elsewhere) and s = sum_live c^2 (rho(ru) + rho(rv)), columns in
// ascending order.  live iff c > 0 (false for 0, negatives and NaN), the row is a joint the stage poses and its depth Z > z_near (false for
// NaN); a dead entry's keypoint is never read.  sigma2 = sigma^2, or 0 for no robustifier.
//   ru = f (X / Z) - (k_u - centre_u);  rho(r) = sigma2 r^2 / (sigma2 + r^2);  1/2 rho'(r) = (sigma2 / (sigma2 + r^2))^2 r
__global__ void __launch_bounds__(64) k_kg_resid(const float* __restrict__ posed, const float* __restrict__ kp, const float* __restrict__ conf,
                                                 const int32_t* __restrict__ rows, int n_obs, const float* __restrict__ focal,
                                                 const float* __restrict__ center, float sigma2, float z_near, float* __restrict__ dj,
                                                 float* __restrict__ s, int64_t B) {
    const int64_t b = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    float* g = dj + b * JG_ROW;
    for (int k = 0; k < JG_ROW; ++k) g[k] = 0.f;
    const float* P = posed + b * JG_ROW;
    const float f = focal[b], cu = center[2 * b], cv = center[2 * b + 1];
    float acc = 0.f;
    for (int j = 0; j < n_obs; ++j) {
        const int row = rows ? rows[j] : j;
        const float c = conf ? conf[b * n_obs + j] : 1.0f;
        if (!(c > 0.f) || row < 0 || row >= JG_NJ) continue;
        const float X = P[3 * row], Y = P[3 * row + 1], Z = P[3 * row + 2];
        if (!(Z > z_near)) continue;
        const float* k = kp + (b * n_obs + j) * 2;
        const float ru = f * (X / Z) - (k[0] - cu), rv = f * (Y / Z) - (k[1] - cv);
        const float ru2 = ru * ru, rv2 = rv * rv;
        float rho_u = ru2, rho_v = rv2, wu = ru, wv = rv;
        if (sigma2 > 0.f) {
            const float du = sigma2 + ru2, dv = sigma2 + rv2, qu = sigma2 / du, qv = sigma2 / dv;
            rho_u = (sigma2 * ru2) / du; rho_v = (sigma2 * rv2) / dv;
            wu = (qu * qu) * ru; wv = (qv * qv) * rv;
        }
        const float c2 = c * c, fz = f / Z;
        wu *= c2; wv *= c2;
        g[3 * row] = wu * fz; g[3 * row + 1] = wv * fz; g[3 * row + 2] = -((wu * X + wv * Y) * fz) / Z;
        acc += c2 * (rho_u + rho_v);
    }
    s[b] = acc;
}

// the normaliser's scale: d pose / d y0 per column
__global__ void __launch_bounds__(256) k_jg_scale(const float* __restrict__ dpose, int mode, const float* __restrict__ a, const float* __restrict__ b,
                                                  float* __restrict__ v, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c = (int)(i % JG_D);
    float g = dpose[i];
    if (mode == 1) g = g * b[c];
    else if (mode == 2) g = g * (0.5f * (b[c] - a[c]));
    v[i] = g;
}
}  // namespace

// A [B][22][12] | posed [B][66] | d joints [B][66] | pose [B][63] | d pose [B][63], fp32
extern "C" int64_t dposer_joint_guide_stage_scratch_bytes(int64_t batch) {
    return batch < 1 ? 0 : batch * (JG_NJ * 12 + 2 * JG_ROW + 2 * JG_D) * (int64_t)sizeof(float);
}

extern "C" int dposer_joint_guide_stage(dposer_body_t body, const float* y0, int32_t data_dim, int32_t norm_mode, const float* norm_a,
                                        const float* norm_b, const float* root_orient, const float* transl, const float* j_rest,
                                        int32_t j_rest_batched, const float* joints_obs, const float* joints_conf, const int32_t* obs_rows,
                                        int32_t n_obs, float* s, float* v, void* scratch, int64_t batch, void* stream) {
    DP_RANGE();
    DP_CHECK_ARG(body, "null handle");
    DP_CHECK_ARG(y0 && j_rest && joints_obs && s && v, "null argument");
    if (data_dim == 2 * JG_D)
        return dposer_set_error(DPOSER_ERR_UNSUPPORTED, std::string(__func__) + ": a rot6d pose (126 inputs) is not supported: the stage takes 21 axis-angle joints (63)");
    DP_CHECK_ARG(data_dim == JG_D, "data_dim must be 63 (21 body joints, axis-angle)");
    DP_CHECK_ARG(norm_mode == 0 || ((norm_mode == 1 || norm_mode == 2) && norm_a && norm_b), "bad normaliser");
    DP_CHECK_ARG(n_obs >= 1 && n_obs <= JG_NJ, "n_obs must be in 1..22");
    DP_CHECK_ARG(batch > 0, "batch must be positive");
    DP_CHECK_ARG(scratch && ((uintptr_t)scratch & 15) == 0, "scratch must be non-null and 16-byte aligned");
    const int J = body_num_joints(body);
    DP_CHECK_ARG(J > JG_NJ, "the body's tree must hold the 22 body joints first");
    hipStream_t st = (hipStream_t)stream;
    float* A = static_cast<float*>(scratch);
    float* posed = A + batch * JG_NJ * 12;
    float* dj = posed + batch * JG_ROW;
    float* pose = dj + batch * JG_ROW;
    float* dpose = pose + batch * JG_D;
    const int64_t n = batch * JG_D;
    hipLaunchKernelGGL(k_jg_denorm, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, st, y0, norm_mode, norm_a, norm_b, pose, n);
    DP_CHECK_HIP(hipGetLastError());
    // root | 21 body joints | everything else of the tree at rest
    const float* segs[3] = {root_orient, pose, nullptr};
    float* dsegs[3] = {nullptr, dpose, nullptr};
    const int32_t segj[3] = {1, JG_NJ - 1, J - JG_NJ};
    DP_TRY(dposer_fk_joints(body, segs, segj, 3, j_rest, j_rest_batched, transl, posed, A, JG_NJ, batch, stream));
    hipLaunchKernelGGL(k_jg_resid, dim3((unsigned)ceil_div(batch, 64)), dim3(64), 0, st, posed, joints_obs, joints_conf, obs_rows, n_obs, dj, s, batch);
    DP_CHECK_HIP(hipGetLastError());
    DP_TRY(fk_joints_backward_launch(body, segs, segj, 3, j_rest, j_rest_batched, A, dj, JG_ROW, JG_NJ, dsegs, nullptr, batch, st));
    hipLaunchKernelGGL(k_jg_scale, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, st, dpose, norm_mode, norm_a, norm_b, v, n);
    DP_CHECK_HIP(hipGetLastError());
    return DPOSER_OK;
}

// the 3D stage's scratch, used the same way
extern "C" int64_t dposer_keypoint_guide_stage_scratch_bytes(int64_t batch) { return dposer_joint_guide_stage_scratch_bytes(batch); }

extern "C" int dposer_keypoint_guide_stage(dposer_body_t body, const float* y0, int32_t data_dim, int32_t norm_mode, const float* norm_a,
                                           const float* norm_b, const float* root_orient, const float* transl, const float* j_rest,
                                           int32_t j_rest_batched, const float* keypoints, const float* keypoints_conf, const int32_t* obs_rows,
                                           int32_t n_obs, const float* focal, const float* center, float sigma, float z_near, float* s, float* v,
                                           void* scratch, int64_t batch, void* stream) {
    DP_RANGE();
    DP_CHECK_ARG(body, "null handle");
    DP_CHECK_ARG(y0 && j_rest && keypoints && focal && center && s && v, "null argument");
    if (data_dim == 2 * JG_D)
        return dposer_set_error(DPOSER_ERR_UNSUPPORTED, std::string(__func__) + ": a rot6d pose (126 inputs) is not supported: the stage takes 21 axis-angle joints (63)");
    DP_CHECK_ARG(data_dim == JG_D, "data_dim must be 63 (21 body joints, axis-angle)");
    DP_CHECK_ARG(norm_mode == 0 || ((norm_mode == 1 || norm_mode == 2) && norm_a && norm_b), "bad normaliser");
    DP_CHECK_ARG(n_obs >= 1 && n_obs <= JG_NJ, "n_obs must be in 1..22");
    DP_CHECK_ARG(z_near > 0.f && z_near <= 3.0e38f, "z_near must be positive and finite");
    DP_CHECK_ARG(sigma <= 0.f || (sigma >= 1.0e-18f && sigma <= 1.0e18f), "sigma must be <= 0 (no robustifier) or in [1e-18, 1e18]: its square must be a normal float");
    DP_CHECK_ARG(batch > 0, "batch must be positive");
    DP_CHECK_ARG(scratch && ((uintptr_t)scratch & 15) == 0, "scratch must be non-null and 16-byte aligned");
    const int J = body_num_joints(body);
    DP_CHECK_ARG(J > JG_NJ, "the body's tree must hold the 22 body joints first");
    hipStream_t st = (hipStream_t)stream;
    float* A = static_cast<float*>(scratch);
    float* posed = A + batch * JG_NJ * 12;
    float* dj = posed + batch * JG_ROW;
    float* pose = dj + batch * JG_ROW;
    float* dpose = pose + batch * JG_D;
    const int64_t n = batch * JG_D;
    hipLaunchKernelGGL(k_jg_denorm, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, st, y0, norm_mode, norm_a, norm_b, pose, n);
    DP_CHECK_HIP(hipGetLastError());
    // root | 21 body joints | everything else of the tree at rest; transl is the camera translation (SMPLify passes transl = camera_t)
    const float* segs[3] = {root_orient, pose, nullptr};
    float* dsegs[3] = {nullptr, dpose, nullptr};
    const int32_t segj[3] = {1, JG_NJ - 1, J - JG_NJ};
    DP_TRY(dposer_fk_joints(body, segs, segj, 3, j_rest, j_rest_batched, transl, posed, A, JG_NJ, batch, stream));
    hipLaunchKernelGGL(k_kg_resid, dim3((unsigned)ceil_div(batch, 64)), dim3(64), 0, st, posed, keypoints, keypoints_conf, obs_rows, n_obs, focal, center,
                       sigma > 0.f ? sigma * sigma : 0.f, z_near, dj, s, batch);
    DP_CHECK_HIP(hipGetLastError());
    DP_TRY(fk_joints_backward_launch(body, segs, segj, 3, j_rest, j_rest_batched, A, dj, JG_ROW, JG_NJ, dsegs, nullptr, batch, st));
    hipLaunchKernelGGL(k_jg_scale, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, st, dpose, norm_mode, norm_a, norm_b, v, n);
    DP_CHECK_HIP(hipGetLastError());
    return DPOSER_OK;
}
