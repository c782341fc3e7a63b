"""One step of the training optimizer as csrc/kernels_api.h documents it at AdamArgs (losses.py optimize_fn + torch.optim.Adam +
ema.py in one pass), in plain numpy and in a chosen precision: the oracle of tests/test_gpu_optimizer.py.  Test infrastructure; no GPU.

    sq      = sum(g^2) over the whole gradient, before grad_scale (or given from outside: the pre-summed form)
    dropped = sq is not finite: nothing changes
    coef    = grad_scale * min(1, grad_clip / (sqrt(sq) * grad_scale + 1e-6)),   grad_scale alone when grad_clip < 0
    outside the no-gradient ranges:  g' = g coef + weight_decay p,  then torch's single-tensor Adam with the host scalars
                                     step_size = lr / (1 - beta1^t),  bc2_sqrt = sqrt(1 - beta2^t)
    everywhere (ema given):          s -= (1 - decay) (s - p_new)

dtype float64 evaluates this with the python doubles as they are.  dtype float32 rounds every host scalar where csrc/optim_dev.h
(adam_scalars) and csrc/scorefc.hip (fill_adam_args) round it -- formed in double, rounded once -- and evaluates every array operation
in float32, in the order of adam_step / adam_math / adam_prologue (csrc/elementwise.hip).

``mutation`` plants one named fault (MUTATIONS): what a subtly wrong kernel would compute.  tests/test_adam_ref_cpu.py shows that each
leaves the comparison band of tests/adam_cases.py.
"""
import math

import numpy as np

TRIP = 1 << 20          # elements per grid-stride trip: k_sqnorm 1024 blocks x 256 float4 lanes, k_adam_ema 4096 blocks x 256 elements

MUTATIONS = (
    "clip_eps_dropped",             # coef = clip / total_norm
    "clamp_dropped",                # the coefficient is not clamped to 1
    "norm_not_scaled",              # the norm in the coefficient is that of the unscaled gradient
    "wd_before_clip",               # (g + wd p) coef
    "step_minus_1",                 # bias corrections of step t - 1
    "bc2_not_sqrt",                 # sqrt(v) / bc2
    "eps_inside_sqrt",              # sqrt(v + eps) / bc2_sqrt
    "eps_before_bc2",               # (sqrt(v) + eps) / bc2_sqrt
    "ema_from_old_p",               # the shadow follows the parameter from before the step
    "ema_skipped_in_nograd",        # no shadow update inside a no-gradient range
    "adam_in_nograd",               # Adam runs inside a no-gradient range
    "v_from_unclipped",             # the second moment takes the raw gradient
    "tail_missing_from_norm",       # the n % 4 tail is not in the squared norm
    "second_trip_missing_from_norm",    # k_sqnorm's float4 lanes stop after one grid-stride trip
    "second_trip_untouched",        # k_adam_ema stops after one grid-stride trip: elements from 2^20 on stay as they are
    "coef_without_grad_scale",      # the clip coefficient is applied, grad_scale is not
)


def host_scalars(dtype, lr, beta1, beta2, eps, step):
    """adam_scalars (csrc/optim_dev.h): formed in double, converted once."""
    T = np.dtype(dtype).type
    bc1, bc2 = 1.0 - math.pow(beta1, step), 1.0 - math.pow(beta2, step)
    with np.errstate(divide="ignore"):
        step_size = T(np.float64(lr) / np.float64(bc1))
    return dict(step_size=step_size, one_minus_beta1=T(1.0 - beta1), beta2=T(beta2), one_minus_beta2=T(1.0 - beta2),
                bc2_sqrt=T(math.sqrt(bc2)), bc2=T(bc2), eps=T(eps))


def squared_norm(g, dtype=np.float64, mutation=None):
    g = np.asarray(g, dtype=dtype)
    n = g.size
    if mutation == "tail_missing_from_norm":
        g = g[:n - (n & 3)]
    elif mutation == "second_trip_missing_from_norm":
        g = np.concatenate([g[:min(n - (n & 3), TRIP)], g[n - (n & 3):]])
    # a fixed tree of elementwise additions (zero-padded to a power of two, halves added until one entry is left): every addition is
    # one IEEE operation of ``dtype``, so the float32 sum has the same bits on every host (numpy's own reduction picks its order
    # by the vector width of the CPU)
    with np.errstate(over="ignore", invalid="ignore"):
        a = np.zeros(1 << max(g.size - 1, 0).bit_length(), dtype=dtype)
        a[:g.size] = g * g
        while a.size > 1:
            a = a[:a.size // 2] + a[a.size // 2:]
    return np.dtype(dtype).type(a[0])


def adam_step(p, g, m, v, s, skips=(), *, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, grad_clip=-1.0, grad_scale=1.0,
              step, ema_one_minus_decay=0.0, sq=None, dtype=np.float64, mutation=None):
    """-> dict(p, m, v, s (None without a shadow), sq, dropped).  The inputs are not written to."""
    assert mutation is None or mutation in MUTATIONS, mutation
    T = np.dtype(dtype).type
    p, g, m, v = (np.array(a, dtype=dtype) for a in (p, g, m, v))
    s = None if s is None else np.array(s, dtype=dtype)
    n = p.size
    sq = squared_norm(g, dtype, mutation) if sq is None else T(sq)
    if not np.isfinite(sq):
        return dict(p=p, m=m, v=v, s=s, sq=sq, dropped=True)
    gs, clip, wd, omd = T(grad_scale), T(grad_clip), T(weight_decay), T(ema_one_minus_decay)
    coef = gs
    if clip >= 0:
        total_norm = np.sqrt(sq) * (T(1) if mutation == "norm_not_scaled" else gs)
        cc = clip / (total_norm if mutation == "clip_eps_dropped" else total_norm + T(1e-6))
        if mutation != "clamp_dropped" and cc > 1:
            cc = T(1)
        coef = cc if mutation == "coef_without_grad_scale" else gs * cc
    h = host_scalars(dtype, lr, beta1, beta2, eps, step - 1 if mutation == "step_minus_1" else step)

    live = np.ones(n, dtype=bool)
    for lo, hi in skips:
        live[lo:hi] = False
    nograd = ~live
    if mutation == "adam_in_nograd":
        live[:] = True
    if mutation == "second_trip_untouched":
        live[TRIP:] = False
    with np.errstate(all="ignore"):
        gl, pl, ml, vl = g[live], p[live], m[live], v[live]
        if mutation == "wd_before_clip":
            gc = (gl + wd * pl) * coef
        else:
            gc = gl * coef
            if wd != 0:
                gc = gc + wd * pl
        ml = ml + (gc - ml) * h["one_minus_beta1"]
        g2 = gl if mutation == "v_from_unclipped" else gc
        vl = vl * h["beta2"] + h["one_minus_beta2"] * (g2 * g2)
        if mutation == "bc2_not_sqrt":
            denom = np.sqrt(vl) / h["bc2"] + h["eps"]
        elif mutation == "eps_inside_sqrt":
            denom = np.sqrt(vl + h["eps"]) / h["bc2_sqrt"]
        elif mutation == "eps_before_bc2":
            denom = (np.sqrt(vl) + h["eps"]) / h["bc2_sqrt"]
        else:
            denom = np.sqrt(vl) / h["bc2_sqrt"] + h["eps"]
        p_old = p.copy()
        p[live], m[live], v[live] = pl - h["step_size"] * (ml / denom), ml, vl
        if s is not None:
            ema = np.ones(n, dtype=bool)
            if mutation == "ema_skipped_in_nograd":
                ema = ~nograd
            if mutation == "second_trip_untouched":
                ema[TRIP:] = False
            src = p_old if mutation == "ema_from_old_p" else p
            s[ema] = s[ema] - omd * (s[ema] - src[ema])
    assert all(a.dtype == np.dtype(dtype) for a in (p, m, v)) and (s is None or s.dtype == np.dtype(dtype))
    return dict(p=p, m=m, v=v, s=s, sq=sq, dropped=False)
