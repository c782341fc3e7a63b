// dposer_smplify_optimize -- SMPLify.__call__, reference run/smplify.py:182-281 (losses lib/body_model/fitting_losses.py:57-131), as ONE
// C call: the camera stage (num_iters Adam iterations over [global_orient | cam_t]) and the body stage (n_stages x num_iters iterations of
// a fresh Adam over [body_pose | betas | global_orient]) are queued from one loop; nothing returns to the host in between.
//
// Per camera iteration:  LBS forward (rest shape formed once) -> k_sp_cam_grad (camera_fitting_loss gradient into d joints and d cam_t)
//                        -> LBS backward (global-orient segment only) -> k_sp_cam_update (Adam).
// Per body iteration:    shape blend -> LBS forward -> [k_sp_noise] -> dposer_prior_loss_tabled -> k_sp_body_grad (GMoF reprojection)
//                        -> LBS backward (pose segments, rest joints, v_shaped) -> dposer_shape_blend_backward -> k_sp_body_update
//                        (prior through the normaliser, angle and shape priors, Adam, the next iteration's normalised pose).
// The body model is the sub-mesh handle of include/dposer_hip.h: only the vertices the mapped extra joints read are ever skinned.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "common.h"
#include "optim_dev.h"
#include "rng.h"

namespace {

constexpr int kMaxKeypoints = 64;     // one wave per image: one lane per keypoint

__device__ __forceinline__ float wave_sum(float v) {      // butterfly over the 64 lanes: the same order on every call
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fminf(v, __shfl_xor(v, d));
    return v;
}

// normalised network input of every body joint (optim_dev.h pose_norm_joint); one thread per (image, joint)
__global__ void __launch_bounds__(256) k_sp_normalize(const float* body_pose, int NBJ, int mode, const float* a, const float* b, int rot6d,
                                                      float* xn, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t img = i / NBJ;
    const int j = (int)(i % NBJ);
    const int Dn = NBJ * (rot6d ? 6 : 3);
    pose_norm_joint(body_pose + img * NBJ * 3 + j * 3, j, mode, a, b, rot6d != 0, xn + img * Dn, j);
}

// the prior's z when none is injected: Philox keyed by the GLOBAL image index (row0 + b), so a batch split into groups draws the same
// numbers as one call
__global__ void __launch_bounds__(256) k_sp_noise(float* z, int64_t B, int Dn, int64_t row0, uint64_t seed, uint32_t step) {
    const int Dq = (Dn + 3) / 4;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= B * Dq) return;
    const int64_t img = i / Dq;
    const int q = (int)(i % Dq);
    float r[4];
    normals4((uint64_t)(row0 + img) * (uint64_t)Dq + (uint64_t)q, STREAM_PRIOR, step, seed, r);
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (q * 4 + e < Dn) z[img * Dn + q * 4 + e] = r[e];
}

// joints_conf[:, ign_joints] = 0 (smplify.py:238): after the camera stage, in the caller's keypoints
struct IgnList { int32_t idx[8]; int32_t n; };
__global__ void __launch_bounds__(256) k_sp_zero_conf(float* kp, int64_t B, int K, IgnList ign) {
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    for (int i = 0; i < ign.n; ++i) kp[(b * K + ign.idx[i]) * 3 + 2] = 0.f;
}

struct FitArgs {
    const float* joints; int rows;            // LBS joint output [B, rows, 3] (transl = cam_t already added)
    const float* kp; int K;                   // keypoints [B, K, 3]
    const float* focal; const float* center;  // [B], [B, 2]
    const int32_t* jmap; const int32_t* map_ptr; const int32_t* map_entry;
    float* djoints;                           // [B, rows, 3]: the mapped rows are written, the rest stay zero
    float* log4;                              // [B, 4] or NULL
};

// perspective_projection (fitting_losses.py:8-38) with rotation = I: u = f * (x / z) + c_x, v = f * (y / z) + c_y; and its vector-Jacobian
// product for (g_u, g_v)
struct Proj { float x, y, z, u, v, f; };
__device__ __forceinline__ Proj sp_project(const FitArgs& a, int64_t b, int k) {
    Proj p;
    const float* J = a.joints + (b * a.rows + a.jmap[k]) * 3;
    p.x = J[0]; p.y = J[1]; p.z = J[2];
    p.f = a.focal[b];
    p.u = p.f * (p.x / p.z) + a.center[b * 2 + 0];
    p.v = p.f * (p.y / p.z) + a.center[b * 2 + 1];
    return p;
}

// d joints rows from the per-keypoint gradients in LDS: row r = sum of its keypoints' gradients in map order (joint_map has duplicates:
// a scatter would need atomics); returns this lane's share of sum over rows (the gradient of a translation added to every row)
__device__ __forceinline__ float3 sp_rows(const FitArgs& a, int64_t b, const float (*dk)[3]) {
    float3 s = make_float3(0.f, 0.f, 0.f);
    for (int r = threadIdx.x; r < a.rows; r += 64) {
        const int e0 = a.map_ptr[r], e1 = a.map_ptr[r + 1];
        if (e0 == e1) continue;
        float gx = 0.f, gy = 0.f, gz = 0.f;
        for (int e = e0; e < e1; ++e) {
            const int k = a.map_entry[e];
            gx += dk[k][0]; gy += dk[k][1]; gz += dk[k][2];
        }
        float* o = a.djoints + (b * a.rows + r) * 3;
        o[0] = gx; o[1] = gy; o[2] = gz;
        s.x += gx; s.y += gy; s.z += gz;
    }
    return s;
}

struct CamArgs {
    int32_t op[4], gt[4];
    const float* cam_t; const float* cam_t_est;
    float depth_w2;
    float* dcam;                             // [B, 3]
};

// camera_fitting_loss (fitting_losses.py:108-131): sum over the batch of
//   sum_{4 joints} (j2d - proj)^2 of the OP hips / shoulders if all four OP confidences are > 0, else of the four GT joints,
//   + depth_w^2 (t_z - t_z_est)^2.
// One wave per image.  d cam_t = sum over joint rows of d joints (+ the depth term): cam_t is the body model's transl.
__global__ void __launch_bounds__(64) k_sp_cam_grad(FitArgs a, CamArgs c) {
    __shared__ float dk[kMaxKeypoints][3];
    const int64_t b = blockIdx.x;
    const int k = threadIdx.x;
    const float* kp = a.kp + b * a.K * 3;
    float conf_op = INFINITY;
    if (k < 4) conf_op = kp[c.op[k] * 3 + 2];
    const bool valid = wave_min(conf_op) > 0.f;      // is_valid (:124)
    float err = 0.f;
    dk[k][0] = 0.f; dk[k][1] = 0.f; dk[k][2] = 0.f;
    if (k < a.K) {
        bool sel = false;
        for (int i = 0; i < 4; ++i) sel = sel || (valid ? c.op[i] == k : c.gt[i] == k);
        if (sel) {
            const Proj p = sp_project(a, b, k);
            const float ex = kp[k * 3 + 0] - p.u, ey = kp[k * 3 + 1] - p.v;
            err = ex * ex + ey * ey;
            const float gu = -2.f * ex, gv = -2.f * ey;
            const float iz = 1.f / p.z;
            dk[k][0] = gu * p.f * iz;
            dk[k][1] = gv * p.f * iz;
            dk[k][2] = -(gu * p.f * (p.x * iz) + gv * p.f * (p.y * iz)) * iz;
        }
    }
    __syncthreads();
    const float3 s = sp_rows(a, b, dk);
    const float sx = wave_sum(s.x), sy = wave_sum(s.y), sz = wave_sum(s.z);
    const float reproj = wave_sum(err);
    if (k == 0) {
        const float dz = c.cam_t[b * 3 + 2] - c.cam_t_est[b * 3 + 2];
        const float depth = c.depth_w2 * (dz * dz);
        c.dcam[b * 3 + 0] = sx;
        c.dcam[b * 3 + 1] = sy;
        c.dcam[b * 3 + 2] = sz + 2.f * c.depth_w2 * dz;
        if (a.log4) { float* l = a.log4 + b * 4; l[0] = reproj + depth; l[1] = 0.f; l[2] = 0.f; l[3] = depth; }
    }
}

struct BodyArgs {
    float sigma2, inv_batch;
    const float* body_pose; int Db;          // for the loss log: angle prior
    const float* shape; int L, nb;           //                   shape prior
    float w_angle2, w_shape2, w_pose2;
    const float* prior_loss;                 // [1]: sum / batch_size of this call's images
    float* reprojection;                     // final mode: [B, K] conf^2 * GMoF, no gradient
};

// body_fitting_loss (fitting_losses.py:57-105), the reprojection part: conf^2 * (gmof(u - x) + gmof(v - y)), gmof(e) = s^2 e^2 / (s^2 + e^2);
// the batch mean makes every image's gradient 1 / B.  One wave per image; the loss log gets the four weighted terms.
template <bool FINAL> __global__ void __launch_bounds__(64) k_sp_body_grad(FitArgs a, BodyArgs o) {
    __shared__ float dk[kMaxKeypoints][3];
    const int64_t b = blockIdx.x;
    const int k = threadIdx.x;
    const float* kp = a.kp + b * a.K * 3;
    float rl = 0.f;
    dk[k][0] = 0.f; dk[k][1] = 0.f; dk[k][2] = 0.f;
    if (k < a.K) {
        const Proj p = sp_project(a, b, k);
        const float conf = kp[k * 3 + 2];
        const float c2 = conf * conf;
        const float ex = p.u - kp[k * 3 + 0], ey = p.v - kp[k * 3 + 1];
        const float qx = ex * ex, qy = ey * ey;
        const float dx = o.sigma2 + qx, dy = o.sigma2 + qy;
        rl = c2 * ((o.sigma2 * qx) / dx + (o.sigma2 * qy) / dy);
        if (FINAL) o.reprojection[b * a.K + k] = rl;
        else {
            // d gmof / d e = 2 e s^4 / (s^2 + e^2)^2
            const float s4 = o.sigma2 * o.sigma2;
            const float gu = o.inv_batch * c2 * (2.f * ex * s4 / (dx * dx));
            const float gv = o.inv_batch * c2 * (2.f * ey * s4 / (dy * dy));
            const float iz = 1.f / p.z;
            dk[k][0] = gu * p.f * iz;
            dk[k][1] = gv * p.f * iz;
            dk[k][2] = -(gu * p.f * (p.x * iz) + gv * p.f * (p.y * iz)) * iz;
        }
    }
    if (FINAL) return;
    __syncthreads();
    sp_rows(a, b, dk);
    const float reproj = wave_sum(rl);
    if (a.log4 && k == 0) {
        const float* q = o.body_pose + b * o.Db;
        // angle_prior (fitting_losses.py:48-54): exp(pose[[52, 55, 9, 12]] * [1, -1, -1, -1])^2
        const float e0 = expf(q[52]), e1 = expf(-q[55]), e2 = expf(-q[9]), e3 = expf(-q[12]);
        const float ang = ((e0 * e0 + e1 * e1) + e2 * e2) + e3 * e3;
        float sh = 0.f;
        for (int l = 0; l < o.nb; ++l) sh += o.shape[b * o.L + l] * o.shape[b * o.L + l];
        float* l4 = a.log4 + b * 4;
        l4[0] = reproj; l4[1] = o.w_angle2 * ang; l4[2] = o.w_shape2 * sh; l4[3] = o.w_pose2 * o.prior_loss[0];
    }
}

// torch.optim.Adam (optim_dev.h adam_step) on a parameter with its moments in memory
__device__ __forceinline__ float sp_adam(float p, float g, float* m_, float* v_, const AdamScalars& s) {
    float m = *m_, v = *v_;
    p = adam_step(p, g, m, v, s);
    *m_ = m; *v_ = v;
    return p;
}

// camera stage update: Adam over [global_orient | cam_t] (smplify.py:207-208); one thread per image
__global__ void __launch_bounds__(256) k_sp_cam_update(float* orient, float* cam_t, const float* dorient, const float* dcam, float* m, float* v,
                                                       int64_t B, AdamScalars s) {
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
#pragma unroll
    for (int c = 0; c < 3; ++c) orient[b * 3 + c] = sp_adam(orient[b * 3 + c], dorient[b * 3 + c], m + b * 6 + c, v + b * 6 + c, s);
#pragma unroll
    for (int c = 0; c < 3; ++c) cam_t[b * 3 + c] = sp_adam(cam_t[b * 3 + c], dcam[b * 3 + c], m + b * 6 + 3 + c, v + b * 6 + 3 + c, s);
}

struct BodyUpdate {
    float* orient; float* body_pose; float* shape;
    const float* dorient; const float* dbody; const float* dshape; const float* gprior;
    float* m; float* v;                      // [B, P], P = 3 + 3 NBJ + nb: orient | body pose | betas
    float* xn;                               // next iteration's normalised pose or NULL
    const float* na; const float* nb_; int mode, rot6d;
    int NBJ, L, nbetas;
    int64_t n;                               // B * (1 + NBJ + nbetas)
    float w_pose2, w_angle2, w_shape2, inv_batch;
    AdamScalars s;
};

// body stage update (smplify.py:240-263): d body_pose = LBS gradient + w_pose^2 normalise^T(d prior / d x_n) (the prior is the batch's
// sum / batch_size: w^2 / B per image, already in gprior's inv_n) + angle prior; d betas = shape-blend gradient + 2 w_shape^2 betas / B;
// then Adam.  One thread per (image, slot): slot 0 = global orient, 1..NBJ = one body joint (three coordinates: the 6-D chain needs all
// three), then one beta per slot.
__global__ void __launch_bounds__(256) k_sp_body_update(BodyUpdate u) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= u.n) return;
    const int slots = 1 + u.NBJ + u.nbetas;
    const int64_t b = i / slots;
    const int sl = (int)(i % slots);
    const int P = 3 + 3 * u.NBJ + u.nbetas;
    float* m = u.m + b * P;
    float* v = u.v + b * P;
    if (sl == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) u.orient[b * 3 + c] = sp_adam(u.orient[b * 3 + c], u.dorient[b * 3 + c], m + c, v + c, u.s);
        return;
    }
    if (sl > u.NBJ) {
        const int l = sl - 1 - u.NBJ;
        float* beta = u.shape + b * u.L + l;
        const float g = u.dshape[b * u.L + l] + u.inv_batch * (u.w_shape2 * (2.f * beta[0]));
        *beta = sp_adam(*beta, g, m + 3 + 3 * u.NBJ + l, v + 3 + 3 * u.NBJ + l, u.s);
        return;
    }
    const int j = sl - 1;
    float* q = u.body_pose + b * 3 * u.NBJ + j * 3;
    const int Dn = (u.rot6d ? 6 : 3) * u.NBJ;
    float gq[3];
    pose_norm_joint_bwd(u.gprior + b * Dn, j, u.w_pose2, q, j, u.mode, u.na, u.nb_, u.rot6d != 0, gq);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int idx = j * 3 + c;
        float g = u.dbody[b * 3 * u.NBJ + idx] + gq[c];
        // angle prior: d/dp exp(s p)^2 = 2 s exp(s p)^2 on body-pose entries 52 (s = +1), 55, 9, 12 (s = -1)
        const float sgn = idx == 52 ? 1.f : ((idx == 55 || idx == 9 || idx == 12) ? -1.f : 0.f);
        if (sgn != 0.f) {
            const float e = expf(sgn * q[c]);
            g += u.inv_batch * (u.w_angle2 * (2.f * sgn * (e * e)));
        }
        q[c] = sp_adam(q[c], g, m + 3 + idx, v + 3 + idx, u.s);
    }
    if (u.xn) pose_norm_joint(q, j, u.mode, u.na, u.nb_, u.rot6d != 0, u.xn + b * Dn, j);
}

struct Scratch {
    float *vs, *jr, *verts, *joints, *djoints, *dverts, *dorient, *dbody, *dvposed, *djrest, *dshape, *sb, *xn, *gprior, *z, *loss1, *dcam,
          *mc, *vc, *mb, *vb;
    int64_t bytes;
};
Scratch layout(char* base, int64_t B, int V, int J, int rows, int L, int Dn) {
    Scratch s;
    char* p = base;
    auto take = [&](int64_t nfloat) { float* r = (float*)p; p += round_up(nfloat * 4, 256); return r; };
    const int64_t P = 3 + 3 * (int64_t)J + L;      // (bound of the body-stage parameters per image: the body segment has < J joints)
    s.vs = take(B * V * 3); s.jr = take(B * J * 3); s.verts = take(B * V * 3); s.joints = take(B * rows * 3); s.djoints = take(B * rows * 3);
    s.dverts = take(B * V * 3); s.dorient = take(B * 3); s.dbody = take(B * 3 * (int64_t)J); s.dvposed = take(B * V * 3); s.djrest = take(B * J * 3);
    s.dshape = take(B * L); s.sb = take(dposer_shape_blend_scratch_floats(V, L, B)); s.xn = take(B * Dn); s.gprior = take(B * Dn); s.z = take(B * Dn);
    s.loss1 = take(64); s.dcam = take(B * 3); s.mc = take(B * 6); s.vc = take(B * 6); s.mb = take(B * P); s.vb = take(B * P);
    s.bytes = p - base;
    return s;
}

}   // namespace

extern "C" int64_t dposer_smplify_scratch_bytes(int64_t batch, int32_t num_vertices, int32_t num_joints, int32_t joint_rows, int32_t num_shape,
                                                int32_t net_inputs) {
    if (batch <= 0 || num_vertices <= 0 || num_joints <= 0 || joint_rows < num_joints || num_shape <= 0 || net_inputs <= 0) return -1;
    return layout(nullptr, batch, num_vertices, num_joints, joint_rows, num_shape, net_inputs).bytes;
}

extern "C" int dposer_smplify_optimize(const dposer_smplify_args* a, void* stream) {
    DP_RANGE();
    DP_CHECK_ARG(a, "null argument");
    DP_CHECK_ARG(a->net && a->flat_params && a->packed && a->net_ws && a->sde && a->freq && a->sigmas, "null score-network argument");
    DP_CHECK_ARG(a->body && a->lbs_ws_fwd && a->lbs_ws_bwd && a->posedirs_packed && a->posedirs_bwd_packed && a->v_template && a->shapedirs &&
                     a->j_template && a->jdirs && a->skin_idx && a->skin_w && a->joint_ptr && a->joint_vidx && a->joint_w && a->segment_joints_host,
                 "null body-model argument");
    DP_CHECK_ARG(a->joint_map && a->map_ptr && a->map_entry && a->keypoints && a->focal_length && a->camera_center && a->cam_t_est &&
                     a->global_orient && a->body_pose && a->shape && a->cam_t && a->scratch && a->reprojection, "null problem argument");
    DP_CHECK_ARG(a->num_iters >= 0 && a->n_stages >= 0 && (a->num_iters * a->n_stages == 0 || a->t_host) &&
                     (a->n_stages == 0 || (a->w_pose_host && a->w_shape_host && a->w_angle_host)), "null / bad schedule");
    DP_CHECK_ARG(a->batch >= 1 && a->batch <= 65535, "1 to 65535 images per call (one grid row per pose in the skinning kernels)");
    DP_CHECK_ARG(a->row0 >= 0 && a->inv_batch > 0.f, "bad global batch");
    DP_CHECK_ARG(a->n_keypoints >= 1 && a->n_keypoints <= kMaxKeypoints, "1 to 64 keypoints (one wave per image)");
    DP_CHECK_ARG(a->num_segments >= 2 && a->num_segments <= 8 && a->orient_segment >= 0 && a->orient_segment < a->num_segments &&
                     a->body_segment >= 0 && a->body_segment < a->num_segments && a->orient_segment != a->body_segment &&
                     a->segment_joints_host[a->orient_segment] == 1, "bad pose segments");
    DP_CHECK_ARG(a->norm_mode == 0 || ((a->norm_mode == 1 || a->norm_mode == 2) && a->norm_a && a->norm_b), "bad normaliser");
    DP_CHECK_ARG(a->num_vertices > 0 && a->num_joints > 0 && a->joint_rows >= a->num_joints && a->num_shape >= 1 && a->num_betas >= 0 &&
                     a->num_betas <= a->num_shape, "bad body-model sizes");
    DP_CHECK_ARG(a->n_ign >= 0 && a->n_ign <= 8, "at most 8 ignored joints");
    for (int i = 0; i < 4; ++i)
        DP_CHECK_ARG(a->op_joints[i] >= 0 && a->op_joints[i] < a->n_keypoints && a->gt_joints[i] >= 0 && a->gt_joints[i] < a->n_keypoints,
                     "camera-loss joints outside the keypoints");
    for (int i = 0; i < a->n_ign; ++i) DP_CHECK_ARG(a->ign_joints[i] >= 0 && a->ign_joints[i] < a->n_keypoints, "ignored joint outside the keypoints");
    DP_CHECK_ARG(((uintptr_t)a->scratch & 255) == 0, "scratch must be 256-byte aligned");
    const int NBJ = a->segment_joints_host[a->body_segment];
    DP_CHECK_ARG(NBJ * 3 > 55, "the body segment must hold the angle prior's pose entries (52, 55, 9, 12)");
    const bool rot6d = a->rot6d != 0;
    const int Dn = NBJ * (rot6d ? 6 : 3);
    {   // the network's input width must be the representation's: noise and prior gradient are indexed with it
        const int64_t wn = dposer_scorefc_tensor_numel(a->net, 0), bn = dposer_scorefc_tensor_numel(a->net, 1);
        DP_CHECK_ARG(wn > 0 && bn > 0 && wn / bn == Dn, "the score network's input width is not the pose representation's (3 J axis-angle, 6 J with rot6d)");
    }
    hipStream_t st = (hipStream_t)stream;
    const int64_t B = a->batch;
    const int V = a->num_vertices, J = a->num_joints, rows = a->joint_rows, L = a->num_shape, K = a->n_keypoints;
    Scratch s = layout((char*)a->scratch, B, V, J, rows, L, Dn);
    const int n_body = a->num_iters * a->n_stages;

    const float* segs[8];
    float* dsegs[8];
    for (int i = 0; i < 8; ++i) { segs[i] = nullptr; dsegs[i] = nullptr; }
    segs[a->orient_segment] = a->global_orient;
    segs[a->body_segment] = a->body_pose;
    dsegs[a->orient_segment] = s.dorient;
    const int64_t P = 3 + 3 * (int64_t)NBJ + a->num_betas;
    DP_CHECK_HIP(hipMemsetAsync(s.djoints, 0, (size_t)B * rows * 3 * 4, st));     // rows no keypoint maps to stay zero
    DP_CHECK_HIP(hipMemsetAsync(s.dverts, 0, (size_t)B * V * 3 * 4, st));         // no loss term reads vertices
    DP_CHECK_HIP(hipMemsetAsync(s.mc, 0, (size_t)B * 6 * 4, st));
    DP_CHECK_HIP(hipMemsetAsync(s.vc, 0, (size_t)B * 6 * 4, st));
    DP_CHECK_HIP(hipMemsetAsync(s.mb, 0, (size_t)B * P * 4, st));
    DP_CHECK_HIP(hipMemsetAsync(s.vb, 0, (size_t)B * P * 4, st));

    FitArgs fa;
    fa.joints = s.joints; fa.rows = rows; fa.kp = a->keypoints; fa.K = K; fa.focal = a->focal_length; fa.center = a->camera_center;
    fa.jmap = a->joint_map; fa.map_ptr = a->map_ptr; fa.map_entry = a->map_entry; fa.djoints = s.djoints; fa.log4 = nullptr;
    auto lbs_fwd = [&]() {
        return dposer_lbs_forward(a->body, a->lbs_ws_fwd, a->posedirs_packed, segs, a->segment_joints_host, a->num_segments, s.jr, 1, s.vs, 1,
                                  a->skin_idx, a->skin_w, a->skin_k, a->cam_t, a->extra_vertex_ids, nullptr, nullptr, s.verts, s.joints, B, stream);
    };

    // ---- camera stage (smplify.py:200-222): betas and body pose fixed, the rest shape formed once
    DP_TRY(dposer_shape_blend_forward(a->v_template, a->shapedirs, a->j_template, a->jdirs, a->shape, s.vs, s.jr, V, J, L, B, stream));
    CamArgs ca;
    for (int i = 0; i < 4; ++i) { ca.op[i] = a->op_joints[i]; ca.gt[i] = a->gt_joints[i]; }
    ca.cam_t = a->cam_t; ca.cam_t_est = a->cam_t_est; ca.depth_w2 = a->depth_weight * a->depth_weight; ca.dcam = s.dcam;
    for (int k = 0; k < a->num_iters; ++k) {
        DP_TRY(lbs_fwd());
        fa.log4 = a->loss_log ? a->loss_log + (int64_t)k * B * 4 : nullptr;
        hipLaunchKernelGGL(k_sp_cam_grad, dim3((unsigned)B), dim3(64), 0, st, fa, ca);
        DP_CHECK_HIP(hipGetLastError());
        DP_TRY(dposer_lbs_backward_fold(a->body, a->lbs_ws_fwd, a->lbs_ws_bwd, a->posedirs_bwd_packed, segs, a->segment_joints_host, a->num_segments,
                                        s.jr, 1, s.vs, 1, a->skin_idx, a->skin_w, a->skin_k, a->joint_ptr, a->joint_vidx, a->joint_w, s.dverts,
                                        s.djoints, (int64_t)rows * 3, a->fold, dsegs, nullptr, nullptr, B, stream));
        hipLaunchKernelGGL(k_sp_cam_update, dim3((unsigned)ceil_div(B, 256)), dim3(256), 0, st, a->global_orient, a->cam_t, (const float*)s.dorient,
                           (const float*)s.dcam, s.mc, s.vc, B, adam_scalars(a->lr, a->beta1, a->beta2, a->eps, k + 1));
        DP_CHECK_HIP(hipGetLastError());
    }

    // ---- joints_conf[:, ign_joints] = 0 (smplify.py:238)
    IgnList ign;
    for (int i = 0; i < 8; ++i) ign.idx[i] = i < a->n_ign ? a->ign_joints[i] : 0;
    ign.n = a->n_ign;
    if (ign.n) {
        hipLaunchKernelGGL(k_sp_zero_conf, dim3((unsigned)ceil_div(B, 256)), dim3(256), 0, st, a->keypoints, B, K, ign);
        DP_CHECK_HIP(hipGetLastError());
    }

    // ---- body stage (smplify.py:240-263): a fresh Adam over [body_pose | betas | global_orient]
    dsegs[a->body_segment] = s.dbody;
    if (n_body > 0) {
        DP_TRY(dposer_prior_table_build_sde(a->net, a->flat_params, a->packed, a->net_ws, a->sde, a->t_host, n_body, a->freq, B, stream));
        const int64_t nn = B * NBJ;
        hipLaunchKernelGGL(k_sp_normalize, dim3((unsigned)ceil_div(nn, 256)), dim3(256), 0, st, (const float*)a->body_pose, NBJ, a->norm_mode, a->norm_a,
                           a->norm_b, a->rot6d, s.xn, nn);
        DP_CHECK_HIP(hipGetLastError());
    }
    for (int k = 0; k < n_body; ++k) {
        const int stage = k / a->num_iters;
        const float wp = a->w_pose_host[stage], ws = a->w_shape_host[stage], wa = a->w_angle_host[stage];
        DP_TRY(dposer_shape_blend_forward(a->v_template, a->shapedirs, a->j_template, a->jdirs, a->shape, s.vs, s.jr, V, J, L, B, stream));
        DP_TRY(lbs_fwd());
        const float* z = a->noise ? a->noise + (int64_t)k * B * Dn : s.z;
        if (!a->noise) {
            hipLaunchKernelGGL(k_sp_noise, dim3((unsigned)ceil_div(B * ((Dn + 3) / 4), 256)), dim3(256), 0, st, s.z, B, Dn, a->row0, a->seed,
                               a->step0 + (uint32_t)k);
            DP_CHECK_HIP(hipGetLastError());
        }
        // DPoser.DPoser_loss (smplify.py:93-107): sum(w (x - x0_hat)^2) / batch_size with w = 0.5 sqrt(1 + SNR)
        DP_TRY(dposer_prior_loss_tabled(a->net, a->flat_params, a->packed, a->net_ws, a->sde, s.xn, z, a->t_host[k], k, n_body, 1, a->inv_batch,
                                        nullptr, s.gprior, s.loss1, a->seed, a->step0 + (uint32_t)k, a->sigmas, B, stream));
        BodyArgs bo;
        bo.sigma2 = a->sigma * a->sigma; bo.inv_batch = a->inv_batch; bo.body_pose = a->body_pose; bo.Db = 3 * NBJ; bo.shape = a->shape; bo.L = L;
        bo.nb = a->num_betas; bo.w_angle2 = wa * wa; bo.w_shape2 = ws * ws; bo.w_pose2 = wp * wp; bo.prior_loss = s.loss1; bo.reprojection = nullptr;
        fa.log4 = a->loss_log ? a->loss_log + (int64_t)(a->num_iters + k) * B * 4 : nullptr;
        hipLaunchKernelGGL(k_sp_body_grad<false>, dim3((unsigned)B), dim3(64), 0, st, fa, bo);
        DP_CHECK_HIP(hipGetLastError());
        DP_TRY(dposer_lbs_backward_fold(a->body, a->lbs_ws_fwd, a->lbs_ws_bwd, a->posedirs_bwd_packed, segs, a->segment_joints_host, a->num_segments,
                                        s.jr, 1, s.vs, 1, a->skin_idx, a->skin_w, a->skin_k, a->joint_ptr, a->joint_vidx, a->joint_w, s.dverts,
                                        s.djoints, (int64_t)rows * 3, a->fold, dsegs, s.djrest, s.dvposed, B, stream));
        DP_TRY(dposer_shape_blend_backward(a->shapedirs, a->jdirs, s.dvposed, s.djrest, s.dshape, s.sb, V, J, L, B, stream));
        BodyUpdate u;
        u.orient = a->global_orient; u.body_pose = a->body_pose; u.shape = a->shape; u.dorient = s.dorient; u.dbody = s.dbody; u.dshape = s.dshape;
        u.gprior = s.gprior; u.m = s.mb; u.v = s.vb; u.xn = k + 1 < n_body ? s.xn : nullptr; u.na = a->norm_a; u.nb_ = a->norm_b;
        u.mode = a->norm_mode; u.rot6d = a->rot6d; u.NBJ = NBJ; u.L = L; u.nbetas = a->num_betas; u.n = B * (1 + NBJ + a->num_betas);
        u.w_pose2 = wp * wp; u.w_angle2 = wa * wa; u.w_shape2 = ws * ws; u.inv_batch = a->inv_batch; u.s = adam_scalars(a->lr, a->beta1, a->beta2, a->eps, k + 1);
        hipLaunchKernelGGL(k_sp_body_update, dim3((unsigned)ceil_div(u.n, 256)), dim3(256), 0, st, u);
        DP_CHECK_HIP(hipGetLastError());
    }

    // ---- reprojection_loss of the final parameters with the zeroed confidences (smplify.py:266-277)
    DP_TRY(dposer_shape_blend_forward(a->v_template, a->shapedirs, a->j_template, a->jdirs, a->shape, s.vs, s.jr, V, J, L, B, stream));
    DP_TRY(lbs_fwd());
    BodyArgs bo;
    std::memset(&bo, 0, sizeof(bo));
    bo.sigma2 = a->sigma * a->sigma; bo.reprojection = a->reprojection;
    fa.log4 = nullptr;
    hipLaunchKernelGGL(k_sp_body_grad<true>, dim3((unsigned)B), dim3(64), 0, st, fa, bo);
    DP_CHECK_HIP(hipGetLastError());
    return DPOSER_OK;
}
