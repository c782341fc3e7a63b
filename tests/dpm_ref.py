"""Test infrastructure for the few-step sampler (dposer_dpm_sampler): DPM-Solver++ (multistep, data prediction) of orders 1 and 2,
stated in float64 on the CPU oracle (``oracle.score_ref.score_fn`` / ``alpha_sigma`` / ``impute``).

For x_t = alpha_t x_0 + sigma_t z and lambda_t = log(alpha_t / sigma_t), times s_0 > ... > s_n, step i from s = s_i to t = s_{i+1},
h = lambda_t - lambda_s:
    D_i = (x + sigma_s^2 score(x, s)) / alpha_s
    order 1:  x <- (sigma_t / sigma_s) x - alpha_t expm1(-h) D_i
    order 2:  x <- (sigma_t / sigma_s) x - alpha_t expm1(-h) D_i - 1/2 alpha_t expm1(-h) (D_i - D_{i-1}) / r,  r = (lambda_s - lambda_{s_{i-1}}) / h
    effective order min(order, i + 1), with lower_order_final also min(., n - i).
The coefficient arithmetic here is this file's own (it never calls the library's ``dpm_coefficients``: that schedule is under test), and it
keeps the update in the form above rather than in the library's three-coefficient combination.
"""
import math

import numpy as np
import torch

from oracle import score_ref as R


def alpha_sigma(sde, t):
    """(alpha, sigma) of ``sde.alpha_sigma`` at the scalar time t, as python floats (float64 arithmetic)."""
    a, s = sde.alpha_sigma(torch.tensor([float(t)], dtype=torch.float64))
    return float(a.reshape(-1)[0]), float(s.reshape(-1)[0])


def log_snr(sde, t):
    a, s = alpha_sigma(sde, t)
    return math.log(a / s)


def effective_order(order, lower_order_final, i, n):
    eff = min(order, i + 1)
    return min(eff, n - i) if lower_order_final else eff


def step_terms(sde, times, i, order, lower_order_final=True):
    """(sigma_t / sigma_s, -alpha_t expm1(-h), r or None) of step i."""
    n = len(times) - 1
    a_s, s_s = alpha_sigma(sde, times[i])
    a_t, s_t = alpha_sigma(sde, times[i + 1])
    lam_s, lam_t = math.log(a_s / s_s), math.log(a_t / s_t)
    h = lam_t - lam_s
    r = None
    if effective_order(order, lower_order_final, i, n) == 2:
        r = (lam_s - log_snr(sde, times[i - 1])) / h
    return s_t / s_s, -a_t * math.expm1(-h), r


def coefficients(sde, times, order, lower_order_final=True):
    """[n, 3] float64: the update of step i regrouped as c_x x + c_0 D_i + c_1 D_{i-1}."""
    n = len(times) - 1
    out = np.zeros((n, 3), dtype=np.float64)
    for i in range(n):
        ratio, e, r = step_terms(sde, times, i, order, lower_order_final)
        out[i] = (ratio, e, 0.0) if r is None else (ratio, e + 0.5 * e / r, -0.5 * e / r)
    return out


def dpm_sampler(p, sde, x_init, times, order, lower_order_final=True, observation=None, mask=None, noise=None, **fw):
    """The solver on the oracle network.  ``x_init`` [B, D] at times[0]; ``noise`` [n, B, D]: the imputation draw z_i used at s_i (a
    completion imputes the state at s_i before the evaluation at s_i; the state after the last update is not imputed).
    Returns (trajs [n, B, D]: the state after each update, before the next imputation; x at times[-1]; x0_hat = the last D)."""
    x = x_init
    n = len(times) - 1
    trajs, d_prev, d_cur = [], None, None
    for i in range(n):
        vec_s = torch.full((x.shape[0],), float(times[i]), dtype=x.dtype)
        if observation is not None:
            x = R.impute(sde, x, vec_s, observation, mask, noise[i])
        score = R.score_fn(p, sde, x, vec_s, **fw)
        alpha, sigma = sde.alpha_sigma(vec_s)
        d_cur = (x + (sigma ** 2)[:, None] * score) / alpha.to(x.dtype)
        ratio, e, r = step_terms(sde, times, i, order, lower_order_final)
        x_new = ratio * x + e * d_cur
        if r is not None:
            x_new = x_new + 0.5 * e * (d_cur - d_prev) / r
        d_prev, x = d_cur, x_new
        trajs.append(x)
    return torch.stack(trajs, 0), x, d_cur
