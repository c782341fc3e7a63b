// The arithmetic the fitting loops share (completion, motion denoising, SMPLify, the training step): torch.optim.Adam's element update
// with its host scalars, and the pose normaliser with its transpose, per coordinate and per joint.  Every user builds with
// -ffp-contract=off: the expressions below are torch's unfused fp32 operations term for term, and their bits are held by the float64
// oracles under tests/: the fitting loops by oracle/task_loops.py, the training step's optimizer (k_adam_ema, k_adam_pack) by
// tests/adam_ref.py.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "rot_dev.h"

// ---- torch.optim.Adam, single-tensor arithmetic ------------------------------------------------------------------------------------------
struct AdamScalars { float step_size, one_minus_beta1, beta2, one_minus_beta2, bc2_sqrt, eps; };

// the scalars of optimiser step `step` (counted from 1): python doubles, rounded once
static inline AdamScalars adam_scalars(double lr, double beta1, double beta2, double eps, double step) {
    const double bc1 = 1.0 - std::pow(beta1, step), bc2 = 1.0 - std::pow(beta2, step);
    AdamScalars s;
    s.step_size = (float)(lr / bc1);                        // torch: step_size = lr / bias_correction1
    s.one_minus_beta1 = (float)(1.0 - beta1); s.beta2 = (float)beta2; s.one_minus_beta2 = (float)(1.0 - beta2);
    s.bc2_sqrt = (float)std::sqrt(bc2); s.eps = (float)eps;
    return s;
}

// one element: updates the moments in place, returns the new parameter value (p by reference: a caller that hands over a memory operand
// has it read here, behind the moments, where the loops have always read it)
__device__ __forceinline__ float adam_step(const float& p, float g, float& m, float& v, const AdamScalars& s) {
    m = m + (g - m) * s.one_minus_beta1;                    // exp_avg.lerp_(grad, 1 - beta1)
    v = v * s.beta2 + s.one_minus_beta2 * (g * g);          // exp_avg_sq.mul_(beta2).addcmul_(g, g, 1 - beta2)
    const float denom = sqrtf(v) / s.bc2_sqrt + s.eps;
    return p - s.step_size * (m / denom);                   // param.addcdiv_(exp_avg, denom, value=-step_size)
}

// ---- offline_normalize(from_axis=True) (lib/dataset/AMASS.py:126-137) --------------------------------------------------------------------
// mode 0 identity, 1 z-score (a = mean, b = std), 2 min-max (a = min, b = max); c = column of the statistics
__device__ __forceinline__ float pose_norm(float p, int mode, const float* a, const float* b, int c) {
    if (mode == 1) return (p - a[c]) / b[c];
    if (mode == 2) return 2.0f * (p - a[c]) / (b[c] - a[c]) - 1.0f;
    return p;
}
// its transpose applied to one prior-gradient entry
__device__ __forceinline__ float pose_norm_bwd(float gp, int mode, const float* a, const float* b, int c) {
    if (mode == 1) gp = gp / b[c];
    else if (mode == 2) gp = (gp / (b[c] - a[c])) * 2.0f;
    return gp;
}

// Joint j's axis-angle q[3] as normalised network inputs: its 3 coordinates, or (rot6d) the first two columns of its rotation matrix,
// row-major (R00 R01 R10 R11 R20 R21: lib/utils/transforms.py:238-255).  They are written as joint jo of xn: jo = j when xn is the pose's
// row, 0 when it points at the joint's own inputs.
__device__ __forceinline__ void pose_norm_joint(const float* q, int j, int mode, const float* a, const float* b, bool rot6d, float* xn, int jo) {
    if (rot6d) {
        const Mat3 R = rodrigues(q[0], q[1], q[2]);
        const float six[6] = {R.m[0], R.m[1], R.m[3], R.m[4], R.m[6], R.m[7]};
#pragma unroll
        for (int e = 0; e < 6; ++e) xn[jo * 6 + e] = pose_norm(six[e], mode, a, b, j * 6 + e);
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) xn[jo * 3 + c] = pose_norm(q[c], mode, a, b, j * 3 + c);
    }
}
// The way back: w * (joint j's 3 or 6 prior-gradient entries, joint jo of gp as above) through normalise^T and, with rot6d, the
// vector-Jacobian product of axis-angle -> (R00 R01 R10 R11 R20 R21), to the joint's three axis-angle parameters gq[3].
__device__ __forceinline__ void pose_norm_joint_bwd(const float* gp, int jo, float w, const float* q, int j, int mode, const float* a,
                                                    const float* b, bool rot6d, float* gq) {
    if (rot6d) {
        float g6[6];
#pragma unroll
        for (int e = 0; e < 6; ++e) g6[e] = pose_norm_bwd(gp[jo * 6 + e] * w, mode, a, b, j * 6 + e);
        const float dR[9] = {g6[0], g6[1], 0.f, g6[2], g6[3], 0.f, g6[4], g6[5], 0.f};
        rodrigues_bwd(q[0], q[1], q[2], dR, gq);
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) gq[c] = pose_norm_bwd(gp[jo * 3 + c] * w, mode, a, b, j * 3 + c);
    }
}
