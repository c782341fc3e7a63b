"""The DPoser pose prior as an nn.Module -- counterpart of the reference's ``DPoser`` in
run/smplify.py:17-115 and of the shared ``one_step_denoise`` / ``loss`` maths of
run/completion.py:105-149 and run/motion_denoising.py:99-143.

One prior evaluation = ``dposer_prior_loss``: perturb x_0 at a shared time t, one forward-only
network evaluation (x0_hat is detached in the reference, so no gradient ever flows through the
network), Tweedie estimate, weighted L2 -- with the analytic gradient 2 w (x_0 - x0_hat)/n returned
to autograd.
"""
import torch
from torch import nn

from . import _C
from .algorithms.advanced import sde_lib
from .algorithms.advanced.model import ScoreModelFC
from .algorithms.ema import ExponentialMovingAverage
from .dataset.AMASS import N_POSES, Posenormalizer
from .tasks._fused import ScoreNetCall, float_array


class _PriorLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x0, model, sde, t, weighted, inv_n, z, seed, step, continuous=True):
        _C.require_gpu(x0, "prior-loss input")
        B = x0.shape[0]
        net = ScoreNetCall(model, sde, continuous, B, 1, x0.device)
        x = x0.detach().contiguous().float()
        grad = torch.empty_like(x)
        x0_hat = torch.empty_like(x)
        loss = torch.empty(1, dtype=torch.float32, device=x.device)
        zz = None if z is None else z.contiguous().float()
        _C.check(net.eng.lib.dposer_prior_loss(*net.head(), _C.ptr(x), _C.ptr(zz), float(t), 1 if weighted else 0, float(inv_n), _C.ptr(x0_hat),
                                               _C.ptr(grad), _C.ptr(loss), int(seed), int(step) & 0xFFFFFFFF, *net.tail(), B, _C.stream_ptr()),
                 "dposer_prior_loss")
        ctx.save_for_backward(grad)
        ctx.x0_hat = x0_hat
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return (grad * g, None, None, None, None, None, None, None, None, None)


def _prior_loss_unfused(model, sde, x0, t, weighted, inv_n, z, continuous=True):
    """smplify.py:93-107 / completion.py:131-149 step by step for an SDE the fused kernel does not cover (VE).  The one-step estimate is
    detached in the reference (smplify.py:73), so the gradient reaches x0 through the explicit (x0 - x0_hat) only."""
    from .algorithms.advanced import utils as mutils
    B = x0.shape[0]
    with torch.no_grad():
        vec_t = torch.full((B,), t, device=x0.device, dtype=torch.float32)
        zz = torch.randn_like(x0) if z is None else z.to(x0.device, torch.float32)
        mean, std = sde.marginal_prob(x0.detach().float(), vec_t)
        x_t = mean + std[:, None] * zz
        score = mutils.get_score_fn(sde, model, train=False, continuous=continuous)(x_t, vec_t, condition=None, mask=None)
        alpha, sigma = sde.return_alpha_sigma(vec_t)
        alpha, sigma = alpha.to(x0.device), sigma.to(x0.device)
        x0_hat = (x_t + (sigma ** 2)[:, None] * score) / alpha              # alpha: [1, 1] (VE) or [B, 1]
        snr = alpha / sigma[:, None]
        w = 0.5 * torch.sqrt(1 + snr) if weighted else torch.full_like(snr, 0.5)
    return (w * (x0.float() - x0_hat) ** 2).sum() * inv_n


MAX_MULTI_DENOISE = 64      # n_steps range of dposer_prior_loss_multi


def multi_step_time_grid(t, n_steps, t_end=None):
    """The reference's time grid ``linear_interpolation(t, t_end, N + 1)`` with ``t_end = t / (2 N)`` (completion.py:113,138), evaluated
    with the reference's own fp32 torch expressions on the host: the N + 1 times carry the reference's bits.  Returns python floats."""
    from .utils.misc import linear_interpolation
    a = torch.tensor([float(t)], dtype=torch.float32)
    b = a / (2 * n_steps) if t_end is None else torch.tensor([float(t_end)], dtype=torch.float32)
    return [float(v) for v in linear_interpolation(a, b, n_steps + 1)[:, 0]]


def _fused_variant_desc(model, sde, continuous):
    """The C descriptor when the one-call variants run (ScoreModelFC under the sub-VP, VP or VE SDE with the continuous score function), else
    None: discrete score functions, other SDEs and other models take the unfused compositions."""
    if not (continuous and isinstance(model, ScoreModelFC)):
        return None
    return sde_lib.sde_desc(sde, True)


def multi_step_prior_eval(model, sde, x0, traj, *, weighted, inv_n, z=None, seed=0, step=0, x0_hat=None, grad=None):
    """One ``dposer_prior_loss_multi`` call along the times ``traj`` (N + 1 python floats): returns ``(loss [1], grad, x0_hat)``, all
    device tensors.  ``x0_hat`` / ``grad``: optional contiguous fp32 [B, D] tensors to write into."""
    _C.require_gpu(x0, "prior-loss input")
    n_steps = len(traj) - 1
    net = ScoreNetCall(model, sde, True, x0.shape[0], n_steps, x0.device)
    x = x0.detach().contiguous().float()
    B = x.shape[0]
    grad = torch.empty_like(x) if grad is None else grad
    x0_hat = torch.empty_like(x) if x0_hat is None else x0_hat
    loss = torch.empty(1, dtype=torch.float32, device=x.device)
    zz = None if z is None else z.detach().to(x.device).contiguous().float()
    _C.check(net.eng.lib.dposer_prior_loss_multi(*net.head(), _C.ptr(x), _C.ptr(zz), float_array(traj), n_steps, 1 if weighted else 0, float(inv_n),
                                                 _C.ptr(x0_hat), _C.ptr(grad), _C.ptr(loss), int(seed), int(step) & 0xFFFFFFFF, *net.tail(), B,
                                                 _C.stream_ptr()), "dposer_prior_loss_multi")
    return loss, grad, x0_hat


def red_diff_eval(model, sde, x0, t, *, z=None, seed=0, step=0, eps_pred=None, grad=None):
    """One ``dposer_prior_red_diff`` call: returns ``(loss [1], grad, eps_pred)``, all device tensors; ``eps_pred`` / ``grad`` as above."""
    _C.require_gpu(x0, "RED-Diff input")
    net = ScoreNetCall(model, sde, True, x0.shape[0], 1, x0.device)
    x = x0.detach().contiguous().float()
    B = x.shape[0]
    grad = torch.empty_like(x) if grad is None else grad
    eps_pred = torch.empty_like(x) if eps_pred is None else eps_pred
    loss = torch.empty(1, dtype=torch.float32, device=x.device)
    zz = None if z is None else z.detach().to(x.device).contiguous().float()
    _C.check(net.eng.lib.dposer_prior_red_diff(*net.head(), _C.ptr(x), _C.ptr(zz), float(t), 1.0 / float(B), _C.ptr(eps_pred), _C.ptr(grad),
                                               _C.ptr(loss), int(seed), int(step) & 0xFFFFFFFF, *net.tail(), B, _C.stream_ptr()),
             "dposer_prior_red_diff")
    return loss, grad, eps_pred


class _PriorLossMulti(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x0, model, sde, traj, weighted, inv_n, z, seed, step):
        loss, grad, _ = multi_step_prior_eval(model, sde, x0, traj, weighted=weighted, inv_n=inv_n, z=z, seed=seed, step=step)
        ctx.save_for_backward(grad)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return (grad * g, None, None, None, None, None, None, None, None)


class _RedDiff(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x0, model, sde, t, z, seed, step):
        loss, grad, _ = red_diff_eval(model, sde, x0, t, z=z, seed=seed, step=step)
        ctx.save_for_backward(grad)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return (grad * g, None, None, None, None, None, None)


def _perturb_unfused(sde, x0, t, z):
    B = x0.shape[0]
    vec_t = torch.full((B,), t, device=x0.device, dtype=torch.float32)
    zz = torch.randn_like(x0, dtype=torch.float32) if z is None else z.to(x0.device, torch.float32)
    mean, std = sde.marginal_prob(x0.detach().float(), vec_t)
    return vec_t, zz, std, mean + std[:, None] * zz


def _prior_loss_multi_unfused(model, sde, x0, traj, weighted, inv_n, z, continuous=True):
    """multi_step_denoise + the loss of completion.py:112-149 step by step: N calls of the HIP score function (``get_score_fn``) and the
    reference's torch elementwise operations.  What runs for models / SDEs / score functions outside the one-call entry."""
    from .algorithms.advanced import utils as mutils
    dev = x0.device
    with torch.no_grad():
        vec_t, _, _, x = _perturb_unfused(sde, x0, traj[0], z)
        score_fn = mutils.get_score_fn(sde, model, train=False, continuous=continuous)
        vec = lambda t: torch.full_like(vec_t, t)
        for i in range(len(traj) - 1):
            t_c = vec(traj[i])
            a_c, s_c = (v.to(dev) for v in sde.return_alpha_sigma(t_c))
            a_b, s_b = (v.to(dev) for v in sde.return_alpha_sigma(vec(traj[i + 1])))
            noise = -score_fn(x, t_c, condition=None, mask=None) * s_c[:, None]
            x = a_b / a_c * (x - s_c[:, None] * noise) + s_b[:, None] * noise
        alpha, sigma = (v.to(dev) for v in sde.return_alpha_sigma(vec_t))
        snr = alpha / sigma[:, None]
        w = 0.5 * torch.sqrt(1 + snr) if weighted else torch.full_like(snr, 0.5)
    return (w * (x0.float() - x) ** 2).sum() * inv_n


def _red_diff_unfused(model, sde, x0, t, z, continuous=True):
    """motion_denoising.py:145-154 step by step over the HIP score function."""
    from .algorithms.advanced import utils as mutils
    dev = x0.device
    with torch.no_grad():
        vec_t, zz, std, x_t = _perturb_unfused(sde, x0, t, z)
        score = mutils.get_score_fn(sde, model, train=False, continuous=continuous)(x_t, vec_t, condition=None, mask=None)
        alpha, sigma = (v.to(dev) for v in sde.return_alpha_sigma(vec_t))
        resid = -score * std[:, None] - zz
        weight = torch.sqrt(sigma ** 2) / alpha[:, 0]
    return torch.mean(weight * torch.einsum("ij,ij->i", resid, x0.float()))


def prior_loss(model, sde, x0, t, *, weighted=True, reduction="mean", batch_size=None, z=None, seed=0, step=0, continuous=True,
               multi_denoise=0, t_end=None):
    """Weighted denoising loss at one shared time ``t`` (python float).
    reduction='mean' -> torch.mean over [B, D] (completion.py:147); 'sum_over_batch' -> sum / batch_size (smplify.py:105).
    ``continuous``: ``config.training.continuous`` as the reference hands it to ``get_score_fn`` (motion_denoising.py:94,
    completion.py:103).  Under the VE SDE it selects the label the network is conditioned on (utils.py:164-181: sigma(t), or
    round((T - t)(N - 1)) for a discrete model), under the VP SDE label and std of the score (utils.py:152-160) -- all on the fused kernel
    since round 6 (DPOSER_SDE_VE_DISCRETE / DPOSER_SDE_VP_DISCRETE).
    ``multi_denoise = N`` (an integer 1..64; the flag ``True`` is refused -- the methods below map it to the reference's 5 / 10): the
    loss on the estimate of N deterministic DDIM steps from ``t`` to ``t_end``
    (default ``t / (2 N)``) instead of the one-step Tweedie estimate -- the reference's ``multi_denoise=True`` branch (completion.py:112-149).
    ONE call of ``dposer_prior_loss_multi`` for a ScoreModelFC under the sub-VP / VP / VE SDE with the continuous score function; discrete
    score functions, other SDEs and other models run ``_prior_loss_multi_unfused``: N calls of the HIP score function and torch elementwise
    operations.  ``multi_denoise`` 0 / False is the one-step call, unchanged."""
    if x0.shape[0] == 0:
        raise ValueError("prior_loss: empty batch (the reference's torch.mean over no elements is NaN)")
    if multi_denoise is True:
        raise ValueError("prior_loss: multi_denoise is the NUMBER of DDIM steps here (the reference's multi_denoise=True is 5 in smplify.py:100, "
                         "10 in completion.py:138 / motion_denoising.py:132: DPoser.DPoser_loss, DPoserComp.loss and MotionDenoise.DPoser_loss take the flag)")
    n_multi = int(multi_denoise)
    if n_multi != multi_denoise or n_multi < 0 or n_multi > MAX_MULTI_DENOISE:
        raise ValueError(f"prior_loss: multi_denoise must be an integer in 0..{MAX_MULTI_DENOISE}, got {multi_denoise!r}")
    n = x0.numel() if reduction == "mean" else (batch_size if batch_size is not None else x0.shape[0])
    if n_multi:
        traj = multi_step_time_grid(t, n_multi, t_end)
        if _fused_variant_desc(model, sde, bool(continuous)) is None:
            return _prior_loss_multi_unfused(model, sde, x0, traj, bool(weighted), 1.0 / float(n), z, continuous=bool(continuous))
        return _PriorLossMulti.apply(x0, model, sde, traj, bool(weighted), 1.0 / float(n), z, seed, step)
    if sde_lib.sde_desc(sde, bool(continuous)) is None:   # not covered by the fused kernel: the HIP score function + the reference's few elementwise steps
        return _prior_loss_unfused(model, sde, x0, float(t), bool(weighted), 1.0 / float(n), z, continuous=bool(continuous))
    return _PriorLoss.apply(x0, model, sde, float(t), bool(weighted), 1.0 / float(n), z, seed, step, bool(continuous))


def red_diff(model, sde, x0, t, *, z=None, seed=0, step=0, continuous=True):
    """The RED-Diff regulariser of motion_denoising.py:145-154 at one shared time ``t``:
    ``mean_b(sigma / alpha * <(eps_pred - z).detach(), x_0>)`` with ``eps_pred = -score * std``; its gradient w.r.t. ``x0`` is
    ``sigma / alpha * (eps_pred - z) / B``.  ONE call of ``dposer_prior_red_diff`` for a ScoreModelFC under the sub-VP / VP / VE SDE with the
    continuous score function (``z=None``: in-kernel noise keyed by ``(seed, step)``); otherwise ``_red_diff_unfused`` over the HIP score
    function."""
    if x0.shape[0] == 0:
        raise ValueError("red_diff: empty batch (the reference's torch.mean over no elements is NaN)")
    if _fused_variant_desc(model, sde, bool(continuous)) is None:
        return _red_diff_unfused(model, sde, x0, float(t), z, continuous=bool(continuous))
    return _RedDiff.apply(x0, model, sde, float(t), z, seed, step)


class DPoser(nn.Module):
    """run/smplify.py:17-115.  ``forward(poses, betas, quan_t)`` returns the prior loss."""

    def __init__(self, batch_size=32, config_path="", args=None, model=None, normalizer=None):
        super().__init__()
        from .utils.generic import import_configs
        self.device = args.device
        self.batch_size = batch_size
        config = import_configs(config_path)
        self.Normalizer = normalizer if normalizer is not None else Posenormalizer(
            data_path=f"{args.dataset_folder}/{args.version}/train", min_max=config.data.min_max,
            rot_rep=config.data.rot_rep, device=args.device)
        diffusion_model = model if model is not None else self.load_model(config, args)
        name = config.training.sde.lower()
        if name == "vpsde":
            sde = sde_lib.VPSDE(beta_min=config.model.beta_min, beta_max=config.model.beta_max, N=config.model.num_scales)
        elif name == "subvpsde":
            sde = sde_lib.subVPSDE(beta_min=config.model.beta_min, beta_max=config.model.beta_max, N=config.model.num_scales)
        elif name == "vesde":
            sde = sde_lib.VESDE(sigma_min=config.model.sigma_min, sigma_max=config.model.sigma_max, N=config.model.num_scales)
        else:
            raise NotImplementedError(f"SDE {config.training.sde} unknown.")
        sde.N = args.sde_N
        self.sde = sde
        self.continuous = bool(getattr(config.training, "continuous", True))      # smplify.py:44: the score function's flavour
        self.model = diffusion_model
        self.model.eval()
        self.model.freeze_packed = False
        self.timesteps = torch.linspace(self.sde.T, 1e-3, self.sde.N)       # host copy: t is a launch scalar
        self._calls = 0

    def load_model(self, config, args):
        pose_dim = 3 if config.data.rot_rep == "axis" else 6
        model = ScoreModelFC(config, n_poses=N_POSES, pose_dim=pose_dim, hidden_dim=config.model.HIDDEN_DIM,
                             embed_dim=config.model.EMBED_DIM, n_blocks=config.model.N_BLOCKS)
        model.to(self.device)
        model.eval()
        ckpt = torch.load(args.ckpt_path, map_location={"cuda:0": self.device})
        ema = ExponentialMovingAverage(model.parameters(), decay=config.model.ema_rate)
        model.load_state_dict(ckpt["model_state_dict"])
        ema.load_state_dict(ckpt["ema"])       # loaded but never copied into the model, as in smplify.py:62-67
        return model

    def DPoser_loss(self, x_0, t, z=None, multi_denoise=False):
        """smplify.py:94-107.  ``multi_denoise=True``: x0_hat from 5 DDIM steps down to t / 10 (:100)."""
        self._calls += 1
        return prior_loss(self.model, self.sde, x_0, t, weighted=True, reduction="sum_over_batch", batch_size=self.batch_size,
                          z=z, seed=self.model._rng_seed + 17, step=self._calls, continuous=getattr(self, "continuous", True),
                          **({"multi_denoise": 5} if multi_denoise else {}))      # (off: today's call, argument for argument)

    def forward(self, poses, betas, quan_t, z=None):
        poses = self.Normalizer.offline_normalize(poses[:, :N_POSES * 3], from_axis=True)
        return self.DPoser_loss(poses, float(self.timesteps[int(quan_t)]), z=z)
