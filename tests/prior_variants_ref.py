"""Test infrastructure: the multi-step (DDIM) prior loss and the RED-Diff regulariser on the CPU oracle.

* ``multi_step_prior``: ``oracle.score_ref.multi_step_denoise`` (N steps from t to t / (2 N) on the linear grid) in place of the one-step
  estimate of ``oracle.score_ref.dposer_prior_loss``, under that loss's weight 0.5 sqrt(1 + SNR) with one_step_denoise's SNR = alpha / sigma
  at t (run/completion.py:112-149; smplify.py:94-107 and motion_denoising.py:124-143 are the 'sum_over_batch' reduction).
* ``red_diff``: run/motion_denoising.py:145-154 restated on ``oracle.score_ref.score_fn``.
Both return the analytic gradient w.r.t. x0 (the estimate / the residual is detached in the reference).
"""
import torch

from oracle import score_ref as R


def oracle_sde(kind, g=None, N=1000):
    if kind == "ve":
        return R.VE(float(g["sigma_min"]) if g is not None else 0.01, float(g["sigma_max"]) if g is not None else 50.0, N=N)
    return (R.VP if kind == "vp" else R.SubVP)(N=N)


def _perturb(sde, x0, t, z):
    tt = torch.full((x0.shape[0],), float(t), dtype=x0.dtype)
    mean, std = sde.marginal_prob(x0, tt)
    return tt, std, mean + std[:, None] * z


def multi_step_prior(p, sde, x0, t, z, N, *, weighted=True, reduction="mean", batch_size=None, **fw):
    """Returns (loss, d loss / d x0, x0_hat)."""
    tt, _, x_t = _perturb(sde, x0, t, z)
    _, est = R.multi_step_denoise(p, sde, x_t, tt, tt / (2 * N), N, **fw)
    alpha, sigma = sde.alpha_sigma(tt)
    snr = alpha / sigma[:, None]                                  # one_step_denoise's alpha / sqrt(sigma^2) (completion.py:108 == :128)
    w = 0.5 * torch.sqrt(1 + snr) if weighted else torch.full_like(snr, 0.5)
    n = x0.numel() if reduction == "mean" else (batch_size if batch_size is not None else x0.shape[0])
    return (w * (x0 - est) ** 2).sum() / n, 2 * w * (x0 - est) / n, est


def red_diff(p, sde, x0, t, z, **fw):
    """Returns (guidance, d guidance / d x0, eps_pred)."""
    tt, std, x_t = _perturb(sde, x0, t, z)
    score = R.score_fn(p, sde, x_t, tt, **fw)
    alpha, sigma = sde.alpha_sigma(tt)
    eps = -score * std[:, None]                                   # :150 score to noise prediction
    weight = torch.sqrt(sigma ** 2) / alpha[:, 0]                 # :151-152
    guidance = torch.mean(weight * torch.einsum("ij,ij->i", eps - z, x0))
    return guidance, weight[:, None] * (eps - z) / x0.shape[0], eps


def red_diff_scalar_amplification(eps, z, x0):
    """How far a relative error of the score moves the RED-Diff scalar, relative to the scalar: the larger of a uniform error (|sum e|) and
    three standard deviations of a random-sign one (3 sqrt(sum e^2)), e = eps_pred * x0, over |sum (eps_pred - z) * x0|.  The scalar is
    compared only where this is <= 2 (condition 3 of the golden's generator): signed terms cancel elsewhere."""
    e = (eps * x0).double()
    tot = ((eps - z) * x0).double().sum()
    return max(abs(float(e.sum())), 3.0 * float(torch.sqrt((e ** 2).sum()))) / abs(float(tot))
