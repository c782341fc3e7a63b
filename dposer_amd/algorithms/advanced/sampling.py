"""Samplers -- counterpart of the reference's lib/algorithms/advanced/sampling.py (registries
:33-77, get_sampling_fn :80-124, Predictor/Corrector :127-174, EulerMaruyamaPredictor :177-207,
ReverseDiffusion/Ancestral/None predictors :210-270, LangevinCorrector :273-302, ALD :305-339,
NoneCorrector :342-350, shared update fns :353-372, get_pc_sampler :375-468).

Fast path on MI355X: Euler-Maruyama predictor + 'none' corrector (the shipped configuration,
configs/subvp/amass_scorefc_continuous.py:30-32) on a sub-VP/VP SDE with a ScoreModelFC runs as
``dposer_em_sampler``: the whole N-step loop is enqueued by one C call, the time branch of the
network collapses into a per-step bias table, the predictor update / completion imputation /
re-tiling of x for the next step are fused into one elementwise kernel per step, and noise is
drawn in-kernel (Philox).  With ``probability_flow=True`` (deterministic sampling along the
probability-flow ODE, what run/demo.py's interpolation task decodes latents with) the same predictor
runs as ``dposer_pf_sampler``: the drift's score term is halved and no noise is added or drawn.

Every other registered pair -- the ``reverse_diffusion``, ``ancestral_sampling`` and ``none`` predictors, the ``langevin`` and ``ald``
correctors -- runs as ``dposer_pc_sampler``: the same host loop in the library (the entries above are its Euler-Maruyama + 'none' case),
per step [network + corrector update] x n_steps_each, network + predictor update, each update one elementwise kernel that also does
the completion imputation and re-tiles x (``fused_pc_supported`` / ``fused_pc_sample``).  The discretisations read the SDE object's own ``discrete_betas`` /
``discrete_sigmas`` on the host; the entries of a step travel to the kernels by value.  What stays outside: Langevin under data
parallelism (``fused_pc_langevin_sample``: three calls per step around the all-reduce of the two norm sums), and probability flow with
a corrector, other models or SDEs: the generic loop below on top of the HIP score function.

The MCG and DPS completion samplers (``get_guided_sampler``: the loop over ``update_fn_guide``, sampling.py:191-207) run as
``dposer_guided_sampler``: per step one network evaluation that keeps its activations, the batch-wide residual norm as a fixed-order sum of
block partials, one dgrad-only backward and one update kernel; other models / SDEs step ``update_fn_guide`` in Python.

The few-step sampler (``get_dpm_sampler``, ``config.sampling.method = "dpm"``; no counterpart in the reference beyond the first-order step of
``multi_step_denoise``): DPM-Solver++ (multistep, data prediction) of order 1 or 2 on ``dpm_time_grid`` runs as ``dposer_dpm_sampler`` -- per
step one network evaluation and one update kernel that combines the state with the last two data predictions under three coefficients
from the host's float64 schedule (``dposer_dpm_coefficients``).  A ScoreModelFC under continuous sub-VP / VP / VE; anything else raises.
"""
import abc
import ctypes as C
import functools
import types

import numpy as np
import torch

from ... import _C
from . import sde_lib
from . import utils as mutils
from .utils import get_score_fn

_CORRECTORS = {}
_PREDICTORS = {}


def _registrar(table):
    def register(cls=None, *, name=None):
        def _register(c):
            key = name if name is not None else c.__name__
            if key in table:
                raise ValueError(f"Already registered model with name: {key}")
            table[key] = c
            return c

        return _register if cls is None else _register(cls)

    return register


register_predictor = _registrar(_PREDICTORS)
register_corrector = _registrar(_CORRECTORS)


def get_predictor(name):
    return _PREDICTORS[name]


def get_corrector(name):
    return _CORRECTORS[name]


def get_sampling_fn(config, sde, shape, inverse_scaler, eps, device=None):
    """sampling.py:80-124."""
    if device is None:
        device = config.device
    name = config.sampling.method.lower()
    if name == "ode":
        return get_ode_sampler(sde=sde, shape=shape, inverse_scaler=inverse_scaler, denoise=config.sampling.noise_removal, eps=eps,
                               device=device)
    if name == "dpm":                      # the few-step solver; the config files carry none of its keys
        return get_dpm_sampler(sde=sde, shape=shape, inverse_scaler=inverse_scaler, steps=int(getattr(config.sampling, "dpm_steps", 20)),
                               order=int(getattr(config.sampling, "dpm_order", 2)),
                               skip_type=getattr(config.sampling, "dpm_skip_type", "logSNR"), continuous=config.training.continuous,
                               denoise=config.sampling.noise_removal, eps=eps, device=device)
    if name != "pc":
        raise ValueError(f"Sampler name {config.sampling.method} unknown.")
    return get_pc_sampler(sde=sde, shape=shape, predictor=get_predictor(config.sampling.predictor.lower()),
                          corrector=get_corrector(config.sampling.corrector.lower()), inverse_scaler=inverse_scaler,
                          snr=config.sampling.snr, n_steps=config.sampling.n_steps_each,
                          probability_flow=config.sampling.probability_flow, continuous=config.training.continuous,
                          denoise=config.sampling.noise_removal, eps=eps, device=device)


class Predictor(abc.ABC):
    def __init__(self, sde, score_fn, probability_flow=False):
        super().__init__()
        self.sde = sde
        self.rsde = sde.reverse(score_fn, probability_flow)
        self.score_fn = score_fn

    @abc.abstractmethod
    def update_fn(self, x, t, observation, mask):
        ...


class Corrector(abc.ABC):
    def __init__(self, sde, score_fn, snr, n_steps):
        super().__init__()
        self.sde, self.score_fn, self.snr, self.n_steps = sde, score_fn, snr, n_steps

    @abc.abstractmethod
    def update_fn(self, x, t, observation, mask):
        ...


@register_predictor(name="euler_maruyama")
class EulerMaruyamaPredictor(Predictor):
    """sampling.py:177-207."""

    def update_fn(self, x, t, observation, mask):
        dt = -1.0 / self.rsde.N
        z = torch.randn_like(x)
        drift, diffusion = self.rsde.sde(x, t)
        x_mean = x + drift * dt
        return x_mean + diffusion[:, None] * np.sqrt(-dt) * z, x_mean

    def update_fn_guide(self, x_t, t, observation, mask, condition=None, grad_step=1.0):
        """MCG / DPS style guided step (sampling.py:191-207); needs d score / d x -> differentiable HIP forward."""
        import contextlib
        x_t.requires_grad_()
        dt = -1.0 / self.rsde.N
        z = torch.randn_like(x_t)
        # only d score / d x is ever asked for here: inside input_grad_only() the backward skips the weight-gradient GEMMs
        model = getattr(self.score_fn, "model", None)
        only_x = model.input_grad_only() if hasattr(model, "input_grad_only") else contextlib.nullcontext()
        with only_x:
            drift, diffusion, alpha, sigma_2, score = self.rsde.sde(x_t, t, condition, mask, guide=True)
        y_mean = x_t.detach() + drift.detach() * dt
        y_hat = y_mean + diffusion[:, None] * np.sqrt(-dt) * z
        with torch.enable_grad():
            y0 = (x_t + sigma_2[:, None] * score) / alpha
            norm = torch.norm((observation * mask) - (y0 * mask))
            g = torch.autograd.grad(outputs=norm, inputs=x_t)[0]
            if torch.isnan(g).any():
                raise ValueError("Consider reduce the value of parameter: grad_step={}".format(grad_step))
            y_hat = y_hat - grad_step * g
        return y_hat, y_mean


@register_predictor(name="reverse_diffusion")
class ReverseDiffusionPredictor(Predictor):
    """sampling.py:210-220."""

    def update_fn(self, x, t, observation=None, mask=None):
        f, G = self.rsde.discretize(x, t)
        z = torch.randn_like(x)
        x_mean = x - f
        return x_mean + G[:, None] * z, x_mean


@register_predictor(name="ancestral_sampling")
class AncestralSamplingPredictor(Predictor):
    """sampling.py:223-259 (VE / VP only)."""

    def __init__(self, sde, score_fn, probability_flow=False):
        super().__init__(sde, score_fn, probability_flow)
        if not isinstance(sde, (sde_lib.VPSDE, sde_lib.VESDE)):
            raise NotImplementedError(f"SDE class {sde.__class__.__name__} not yet supported.")
        assert not probability_flow, "Probability flow not supported by ancestral sampling"

    def update_fn(self, x, t, observation=None, mask=None):
        sde = self.sde
        timestep = (t * (sde.N - 1) / sde.T).long()
        score = self.score_fn(x, t)
        noise = torch.randn_like(x)
        if isinstance(sde, sde_lib.VESDE):
            sigma = sde.discrete_sigmas.to(t.device)[timestep]
            adj = torch.where(timestep == 0, torch.zeros_like(t), sde.discrete_sigmas.to(t.device)[timestep - 1])
            x_mean = x + score * (sigma ** 2 - adj ** 2)[:, None]
            std = torch.sqrt((adj ** 2 * (sigma ** 2 - adj ** 2)) / (sigma ** 2))
            return x_mean + std[:, None] * noise, x_mean
        beta = sde.discrete_betas.to(t.device)[timestep]
        x_mean = (x + beta[:, None] * score) / torch.sqrt(1.0 - beta)[:, None]
        return x_mean + torch.sqrt(beta)[:, None] * noise, x_mean


@register_predictor(name="none")
class NonePredictor(Predictor):
    def __init__(self, sde, score_fn, probability_flow=False):
        pass

    def update_fn(self, x, t, observation, mask):
        return x, x


def _langevin_alpha(sde, t):
    if isinstance(sde, (sde_lib.VPSDE, sde_lib.subVPSDE)):
        return sde.alphas.to(t.device)[(t * (sde.N - 1) / sde.T).long()]
    return torch.ones_like(t)


def _check_langevin_sde(sde):
    if not isinstance(sde, (sde_lib.VPSDE, sde_lib.VESDE, sde_lib.subVPSDE)):
        raise NotImplementedError(f"SDE class {sde.__class__.__name__} not yet supported.")


@register_corrector(name="langevin")
class LangevinCorrector(Corrector):
    """sampling.py:273-302.  The step size couples the samples through batch-mean norms (:296-297).  This class is the generic
    form (any score function, means over the tensor it is given); ``pc_sampler`` runs Langevin + Euler-Maruyama on the HIP
    path instead (``fused_pc_langevin_sample``), where the means are GLOBAL-batch means also under data parallelism: the two
    norm sums are all-reduced between the two phases of ``dposer_langevin_step``."""

    def __init__(self, sde, score_fn, snr, n_steps):
        super().__init__(sde, score_fn, snr, n_steps)
        _check_langevin_sde(sde)

    def update_fn(self, x, t, observation, mask):
        alpha = _langevin_alpha(self.sde, t)
        x_mean = x
        for _ in range(self.n_steps):
            grad = self.score_fn(x, t, condition=None, mask=mask)
            noise = torch.randn_like(x)
            grad_norm = torch.norm(grad.reshape(grad.shape[0], -1), dim=-1).mean()
            noise_norm = torch.norm(noise.reshape(noise.shape[0], -1), dim=-1).mean()
            step = (self.snr * noise_norm / grad_norm) ** 2 * 2 * alpha
            x_mean = x + step[:, None] * grad
            x = x_mean + torch.sqrt(step * 2)[:, None] * noise
        return x, x_mean


@register_corrector(name="ald")
class AnnealedLangevinDynamics(Corrector):
    """sampling.py:305-339."""

    def __init__(self, sde, score_fn, snr, n_steps):
        super().__init__(sde, score_fn, snr, n_steps)
        _check_langevin_sde(sde)

    def update_fn(self, x, t, observation, mask):
        alpha = _langevin_alpha(self.sde, t)
        std = self.sde.marginal_prob(x, t)[1]
        x_mean = x
        for _ in range(self.n_steps):
            grad = self.score_fn(x, t, condition=None, mask=mask)
            noise = torch.randn_like(x)
            step = (self.snr * std) ** 2 * 2 * alpha
            x_mean = x + step[:, None] * grad
            x = x_mean + noise * torch.sqrt(step * 2)[:, None]
        return x, x_mean


@register_corrector(name="none")
class NoneCorrector(Corrector):
    def __init__(self, sde, score_fn, snr, n_steps):
        pass

    def update_fn(self, x, t, observation, mask):
        return x, x


def shared_predictor_update_fn(x, t, observation, mask, sde, model, predictor, probability_flow, continuous):
    """sampling.py:353-361."""
    score_fn = mutils.get_score_fn(sde, model, train=False, continuous=continuous)
    obj = NonePredictor(sde, score_fn, probability_flow) if predictor is None else predictor(sde, score_fn, probability_flow)
    return obj.update_fn(x, t, observation, mask)


def shared_corrector_update_fn(x, t, observation, mask, sde, model, corrector, continuous, snr, n_steps):
    """sampling.py:364-372."""
    score_fn = mutils.get_score_fn(sde, model, train=False, continuous=continuous)
    obj = NoneCorrector(sde, score_fn, snr, n_steps) if corrector is None else corrector(sde, score_fn, snr, n_steps)
    return obj.update_fn(x, t, observation, mask)


def fused_em_supported(sde, model, predictor, corrector, probability_flow, continuous):
    """Euler-Maruyama + corrector 'none' on a fused SDE and a ScoreModelFC; ``probability_flow`` selects dposer_pf_sampler."""
    from .model import ScoreModelFC
    return (predictor is EulerMaruyamaPredictor and corrector in (None, NoneCorrector)
            and sde_lib.sde_desc(sde, continuous) is not None
            and isinstance(model, ScoreModelFC))


def _fused_prelude(model, sde, x, timesteps, n_run, traj_stride, continuous, observation, mask, noise, with_backward=False):
    """What the three ``fused_*`` runners set up alike: the engine and its buffers, the state clones, the host timesteps, the trajectory,
    the SDE descriptor and the optional tensors as contiguous fp32.  The workspace is the caller's (its table rows differ)."""
    _C.require_gpu(x, "sampler state")
    p = types.SimpleNamespace(eng=model._engine(), flat=model.flat_params(), B=x.shape[0])
    p.packed = p.eng.packed(p.flat, with_backward=with_backward, force=not model.freeze_packed)
    p.x = x.contiguous().float().clone()
    p.x_mean = p.x.clone()
    p.ts_host = timesteps.detach().to("cpu", torch.float32).contiguous()
    p.traj = torch.empty((n_run // traj_stride,) + tuple(x.shape), dtype=torch.float32, device=x.device) if (traj_stride and n_run > 0) else None
    p.desc = sde_lib.sde_desc(sde, continuous)
    p.obs, p.msk, p.nz = (None if v is None else v.contiguous().float() for v in (observation, mask, noise))
    return p


def fused_em_sample(model, sde, x, timesteps, *, start_step=0, observation=None, mask=None, noise=None, seed=0,
                    traj_stride=0, continuous=True, probability_flow=False):
    """dposer_em_sampler (dposer_pf_sampler with ``probability_flow``).  x [B, D] initial state (consumed); returns
    (trajs or None, x, x_mean).  Under probability flow x == x_mean and ``noise`` keeps the stochastic layout: its predictor
    slots are not read."""
    n_run = int(sde.N) - start_step
    p = _fused_prelude(model, sde, x, timesteps, n_run, traj_stride, continuous, observation, mask, noise)
    if p.B == 0:                    # nothing to sample: the reference's loop runs on empty tensors and returns them
        return p.traj, p.x, p.x_mean
    eng, B = p.eng, p.B
    ws = eng.workspace(B, _C.WS_SHARED_T, max(n_run, 1), x.device)
    name = "dposer_pf_sampler" if probability_flow else "dposer_em_sampler"
    _C.check(getattr(eng.lib, name)(eng.h, _C.ptr(p.flat), _C.ptr(p.packed), _C.ptr(ws), C.byref(p.desc), _C.ptr(p.x), _C.ptr(p.x_mean),
                                    C.c_void_p(p.ts_host.data_ptr()), int(start_step), _C.ptr(p.obs), _C.ptr(p.msk), _C.ptr(p.nz),
                                    int(seed), _C.ptr(p.traj), int(traj_stride or 1), _C.ptr(eng.freq(x.device, model._fourier_W())),
                                    _C.ptr(model.sigmas), B, _C.stream_ptr()), name)
    return p.traj, p.x, p.x_mean


def fused_langevin_supported(sde, model, predictor, corrector, probability_flow, continuous):
    from .model import ScoreModelFC
    return (predictor is EulerMaruyamaPredictor and corrector is LangevinCorrector and not probability_flow
            and sde_lib.sde_desc(sde, continuous) is not None
            and isinstance(model, ScoreModelFC))


def fused_pc_langevin_sample(model, sde, x, timesteps, *, snr, n_steps=1, start_step=0, observation=None, mask=None, noise=None,
                             seed=0, traj_stride=0, continuous=True):
    """Predictor-corrector loop of sampling.py:455-461 with the Langevin corrector (:282-302) and the Euler-Maruyama predictor
    on the HIP path.  Per outer step: ``n_steps`` x [``dposer_langevin_step`` phase 0 -> all-reduce of the two norm sums over
    the data-parallel ranks -> phase 1], then ``dposer_em_sampler_steps`` for the (imputation,) predictor (, imputation) of that
    step.  Nothing synchronises with the host inside the loop.
    ``noise`` [n_run, n_steps + (3 if completion else 1), B, D]: injected draws in the reference's order (tests)."""
    from ... import distributed as ddp
    n_run = int(sde.N) - start_step
    p = _fused_prelude(model, sde, x, timesteps, n_run, traj_stride, continuous, observation, mask, noise)
    # No early return for B == 0 here, unlike the one-call runners: this is the data-parallel path, and a rank with an empty shard
    # still has to take part in every all-reduce below or its peers hang.  What B == 0 does is left as it always was.
    eng, flat, packed, B, x, x_mean, ts_host, traj, desc, obs, msk, nz = (p.eng, p.flat, p.packed, p.B, p.x, p.x_mean, p.ts_host, p.traj, p.desc,
                                                                          p.obs, p.msk, p.nz)
    ws = eng.workspace(B, _C.WS_SHARED_T, 1, x.device)
    k_pred = 3 if obs is not None else 1
    dp = ddp.dp_active()
    global_batch = B
    if dp:                                         # ragged shards: the global batch is the sum of the local ones (once per call)
        cnt = torch.tensor([float(B)], dtype=torch.float64, device=x.device)     # on the device: RCCL cannot reduce a CPU tensor
        ddp.all_reduce_sum_(cnt)
        global_batch = int(cnt.item())
    norms = torch.empty(2, dtype=torch.float32, device=x.device)
    alphas = sde.alphas.detach().to("cpu") if hasattr(sde, "alphas") else None
    freq, lib = eng.freq(x.device, model._fourier_W()), eng.lib
    for i in range(n_run):
        gi = start_step + i
        t = ts_host[gi]
        alpha = float(alphas[int((t * (sde.N - 1) / sde.T).long())]) if alphas is not None else 1.0      # sampling.py:290-294
        for k in range(n_steps):
            z = None if nz is None else nz[i, k]
            args = (eng.h, _C.ptr(flat), _C.ptr(packed), _C.ptr(ws), C.byref(desc), _C.ptr(x), _C.ptr(x_mean), float(t), alpha, float(snr),
                    _C.ptr(z), int(seed), (gi * n_steps + k) & 0xFFFFFFFF, _C.ptr(norms))
            _C.check(lib.dposer_langevin_step(*args, 0, 1.0 / global_batch, _C.ptr(freq), _C.ptr(model.sigmas), B, _C.stream_ptr()),
                     "dposer_langevin_step")
            if dp:
                ddp.all_reduce_sum_(norms)         # two floats: keeps the reference's global-batch means under DP
            _C.check(lib.dposer_langevin_step(*args, 1, 1.0 / global_batch, _C.ptr(freq), _C.ptr(model.sigmas), B, _C.stream_ptr()),
                     "dposer_langevin_step")
        zp = None if nz is None else nz[i, n_steps:n_steps + k_pred].contiguous()
        slot = traj[(i + 1) // traj_stride - 1] if (traj is not None and (i + 1) % traj_stride == 0) else None
        _C.check(lib.dposer_em_sampler_steps(eng.h, _C.ptr(flat), _C.ptr(packed), _C.ptr(ws), C.byref(desc), _C.ptr(x), _C.ptr(x_mean),
                                             C.c_void_p(ts_host.data_ptr()), int(gi), 1, _C.ptr(obs), _C.ptr(msk), _C.ptr(zp), int(seed),
                                             _C.ptr(slot), 1, _C.ptr(freq), _C.ptr(model.sigmas), B, _C.stream_ptr()),
                 "dposer_em_sampler_steps")
    return traj, x, x_mean


_PC_PRED_KINDS = {None: _C.PC_PRED_NONE, NonePredictor: _C.PC_PRED_NONE, EulerMaruyamaPredictor: _C.PC_PRED_EULER_MARUYAMA,
                  ReverseDiffusionPredictor: _C.PC_PRED_REVERSE_DIFFUSION, AncestralSamplingPredictor: _C.PC_PRED_ANCESTRAL}
_PC_CORR_KINDS = {None: _C.PC_CORR_NONE, NoneCorrector: _C.PC_CORR_NONE, LangevinCorrector: _C.PC_CORR_LANGEVIN,
                  AnnealedLangevinDynamics: _C.PC_CORR_ALD}


def _discrete_table(sde):
    """The SDE object's own table that the discretisations index with ``(t * (N - 1) / T).long()``: ``discrete_betas`` (sub-VP / VP,
    ``alphas`` is 1 - it) or ``discrete_sigmas`` (VE); None when it no longer has sde.N entries (N changed after construction)."""
    tab = sde.discrete_sigmas if isinstance(sde, sde_lib.VESDE) else getattr(sde, "discrete_betas", None)
    if tab is None or tab.dim() != 1 or int(tab.shape[0]) != int(sde.N):
        return None
    return tab.detach().to("cpu", torch.float32).contiguous()


def _pc_reads_table(sde, pred, corr):
    """Whether the pair indexes the SDE's discrete table: ancestral sampling, reverse diffusion over the DDPM / SMLD discretisations
    (VP / VE), and alpha of the Langevin / ALD correctors under sub-VP / VP."""
    ve = isinstance(sde, sde_lib.VESDE)
    return (pred == _C.PC_PRED_ANCESTRAL or (pred == _C.PC_PRED_REVERSE_DIFFUSION and not isinstance(sde, sde_lib.subVPSDE))
            or (corr != _C.PC_CORR_NONE and not ve))


def fused_pc_supported(sde, model, predictor, corrector, probability_flow, continuous):
    """What ``dposer_pc_sampler`` takes from pc_sampler: every registered predictor x corrector on a fused SDE and a ScoreModelFC, except
    * Langevin under data parallelism (its batch means need the all-reduce between the two phases: the per-step path keeps it),
    * probability flow with a corrector (generic loop) or with ancestral sampling (the constructor's assertion must surface),
    * ancestral sampling on sub-VP (the constructor's NotImplementedError must surface),
    * a pair that reads the SDE's discrete table when that table no longer has sde.N entries (N changed after construction)."""
    from ... import distributed as ddp
    from .model import ScoreModelFC
    if predictor not in _PC_PRED_KINDS or corrector not in _PC_CORR_KINDS:
        return False
    if not isinstance(model, ScoreModelFC) or sde_lib.sde_desc(sde, continuous) is None:
        return False
    pred, corr = _PC_PRED_KINDS[predictor], _PC_CORR_KINDS[corrector]
    if _pc_reads_table(sde, pred, corr) and _discrete_table(sde) is None:     # (N changed after construction: the table is the constructor's)
        return False
    if probability_flow and (corr != _C.PC_CORR_NONE or pred == _C.PC_PRED_ANCESTRAL):
        return False
    if pred == _C.PC_PRED_ANCESTRAL and not isinstance(sde, (sde_lib.VPSDE, sde_lib.VESDE)):
        return False
    if corr == _C.PC_CORR_LANGEVIN and ddp.dp_active():
        return False
    return True


def fused_pc_sample(model, sde, x, timesteps, *, predictor, corrector, snr=0.16, n_steps=1, probability_flow=False, start_step=0,
                    run_steps=-1, observation=None, mask=None, noise=None, seed=0, traj_stride=0, continuous=True):
    """dposer_pc_sampler: loop indices [start_step, start_step + run_steps) (run_steps < 0: to N) of sampling.py:455-461 for any
    registered predictor / corrector class in ONE library call.  x [B, D] initial state (consumed); returns (trajs or None, x, x_mean).
    ``noise`` [n_run, (n_steps if a corrector) + (3 if completion else 1), B, D]: injected draws in the reference's order (corrector
    draws, impute-after-corrector, predictor z, impute-after-predictor); a slot the algorithm does not read is present and ignored."""
    N = int(sde.N)
    n_run = N - start_step if (run_steps < 0 or run_steps > N - start_step) else int(run_steps)
    p = _fused_prelude(model, sde, x, timesteps, n_run, traj_stride, continuous, observation, mask, noise)
    if p.B == 0:                    # nothing to sample: the reference's loop runs on empty tensors and returns them
        return p.traj, p.x, p.x_mean
    eng, B = p.eng, p.B
    ws = eng.workspace(B, _C.WS_SHARED_T, max(n_run, 1), x.device)
    pc = _C.PcDesc(_PC_PRED_KINDS[predictor], _PC_CORR_KINDS[corrector], int(n_steps), int(bool(probability_flow)), float(snr), 1.0 / B)
    table = _discrete_table(sde) if _pc_reads_table(sde, pc.predictor, pc.corrector) else None
    if table is None and _pc_reads_table(sde, pc.predictor, pc.corrector):
        raise ValueError("the SDE's discrete table no longer has sde.N entries: this predictor / corrector pair cannot run on it")
    norms = torch.empty(2, dtype=torch.float32, device=x.device) if pc.corrector == _C.PC_CORR_LANGEVIN else None
    _C.check(eng.lib.dposer_pc_sampler(eng.h, _C.ptr(p.flat), _C.ptr(p.packed), _C.ptr(ws), C.byref(p.desc), C.byref(pc), _C.ptr(p.x),
                                       _C.ptr(p.x_mean), C.c_void_p(p.ts_host.data_ptr()), int(start_step), int(run_steps), _C.ptr(p.obs),
                                       _C.ptr(p.msk), _C.ptr(p.nz), int(seed), _C.ptr(p.traj), int(traj_stride or 1),
                                       C.c_void_p(table.data_ptr()) if table is not None else None, _C.ptr(norms),
                                       _C.ptr(eng.freq(x.device, model._fourier_W())), _C.ptr(model.sigmas), B, _C.stream_ptr()),
             "dposer_pc_sampler")
    return p.traj, p.x, p.x_mean


def get_pc_sampler(sde, shape, predictor, corrector, inverse_scaler, snr, n_steps=1, probability_flow=False,
                   continuous=False, denoise=True, eps=1e-3, device="cuda"):
    """Predictor-corrector sampler factory (sampling.py:375-468).

    The returned ``pc_sampler(model, observation, mask, z, start_step, args)`` has the reference's
    signature and return value ``(trajs [n, B, D], x_mean if denoise else x)``.  Extra keyword-only
    arguments: ``traj_stride`` (default 1 = every step as the reference; 0 = keep no trajectory --
    at B = 65536, N = 1000 the full tensor is 16.5 GB), ``noise`` (injected draws for tests),
    ``seed`` (Philox key of the in-kernel noise)."""
    def predictor_update_fn(x, t, observation, mask, model):          # (the module-level names: looked up at each call)
        return shared_predictor_update_fn(x, t, observation, mask, sde=sde, model=model, predictor=predictor,
                                          probability_flow=probability_flow, continuous=continuous)

    def corrector_update_fn(x, t, observation, mask, model):
        return shared_corrector_update_fn(x, t, observation, mask, sde=sde, model=model, corrector=corrector, continuous=continuous,
                                          snr=snr, n_steps=n_steps)

    def with_imputation(update_fn):
        def fn(x, vec_t, observation, mask, model, args):
            x, x_mean = update_fn(x, vec_t, observation, mask, model=model)
            if args is not None and args.task in ["completion"]:                 # sampling.py:416-420
                mean, std = sde.marginal_prob(observation, vec_t)
                x = x * (1 - mask) + (mean + torch.randn_like(x) * std[:, None]) * mask
            return x, x_mean

        return fn

    projector = with_imputation(predictor_update_fn)
    correct = with_imputation(corrector_update_fn)
    call_count = [0]

    def pc_sampler(model, observation=None, mask=None, z=None, start_step=0, args=None, *, traj_stride=1, noise=None,
                   seed=None):
        with torch.no_grad():
            # sampling.py:446: the prior is drawn by the SDE (VESDE scales by sigma_max) from torch's CPU generator, so a seeded
            # run starts from the reference's own x_T; callers that keep everything on the device pass z
            x = sde.prior_sampling(shape).to(device) if z is None else z
            timesteps = torch.linspace(sde.T, eps, sde.N, device=device)          # sampling.py:449
            start_t = start_step if (args is not None and args.task in ["denoise"]) else 0
            completion = args is not None and args.task in ["completion"]
            pair = (sde, model, predictor, corrector, probability_flow, continuous)
            runner = None                              # the one-call paths, in this order; each name is looked up at this call
            if fused_em_supported(*pair):
                runner = functools.partial(fused_em_sample, probability_flow=probability_flow)
            elif fused_pc_supported(*pair):
                runner = functools.partial(fused_pc_sample, predictor=predictor, corrector=corrector, snr=snr, n_steps=n_steps,
                                           probability_flow=probability_flow)
            elif fused_langevin_supported(*pair):
                runner = functools.partial(fused_pc_langevin_sample, snr=snr, n_steps=n_steps)
            if runner is not None:
                call_count[0] += 1
                if seed is None:
                    seed = (model._rng_seed * 7919 + call_count[0]) & 0xFFFFFFFFFFFF
                was_training = model.training
                model.eval()                                                       # utils.py:117-119
                trajs, x, x_mean = runner(model, sde, x, torch.linspace(sde.T, eps, sde.N), start_step=start_t,
                                          observation=observation if completion else None, mask=mask if completion else None,
                                          noise=noise, seed=seed, traj_stride=traj_stride, continuous=continuous)
                model.train(was_training)
                if trajs is None:
                    trajs = x.new_empty((0,) + tuple(x.shape))
                return trajs, (x_mean if denoise else x)
            trajs = []
            x_mean = x
            for i in range(start_t, sde.N):
                vec_t = torch.ones(shape[0], device=device) * timesteps[i]
                x, x_mean = correct(x, vec_t, observation, mask, model=model, args=args)
                x, x_mean = projector(x, vec_t, observation, mask, model=model, args=args)
                if traj_stride and (i - start_t + 1) % traj_stride == 0:
                    trajs.append(x)
            trajs = torch.stack(trajs, dim=0) if trajs else x.new_empty((0,) + tuple(x.shape))
            return trajs, (x_mean if denoise else x)

    return pc_sampler


DPM_SKIP_TYPES = ("logSNR", "time_uniform", "time_quadratic")


def _dpm_log_snr(sde, t):
    """lambda(t) = log(alpha_t / sigma_t) in float64, (alpha, sigma) = return_alpha_sigma (sub-VP: sigma = 1 - exp(2 lmc))."""
    t = np.asarray(t, dtype=np.float64)
    if isinstance(sde, sde_lib.VESDE):
        return -(np.log(sde.sigma_min) + t * np.log(sde.sigma_max / sde.sigma_min))
    lmc = -0.25 * t ** 2 * (sde.beta_1 - sde.beta_0) - 0.5 * t * sde.beta_0
    v = -np.expm1(2.0 * lmc)
    return lmc - np.log(v if isinstance(sde, sde_lib.subVPSDE) else np.sqrt(v))


def _dpm_time_of_log_snr(sde, lam):
    """The inverse of ``_dpm_log_snr`` in closed form."""
    lam = np.asarray(lam, dtype=np.float64)
    if isinstance(sde, sde_lib.VESDE):
        return (-lam - np.log(sde.sigma_min)) / np.log(sde.sigma_max / sde.sigma_min)
    if isinstance(sde, sde_lib.subVPSDE):      # e^lambda = alpha / (1 - alpha^2)
        lmc = np.log(2.0) + lam - np.log1p(np.sqrt(1.0 + 4.0 * np.exp(2.0 * lam)))
    else:                                      # VP: alpha^2 + sigma^2 = 1
        lmc = -0.5 * np.logaddexp(0.0, -2.0 * lam)
    b0, db = float(sde.beta_0), float(sde.beta_1 - sde.beta_0)
    L = -lmc                                   # 1/4 db t^2 + 1/2 b0 t = L, the root that stays finite as db -> 0
    return 2.0 * L / (0.5 * b0 + np.sqrt(0.25 * b0 * b0 + db * L))


def dpm_time_grid(sde, steps, skip_type="logSNR", eps=1e-3, T=None):
    """The ``steps + 1`` times s_0 = T > ... > s_steps = eps of the few-step solver, float64.  ``"logSNR"``: uniform in
    lambda = log(alpha / sigma) (what makes 10-30 steps work); ``"time_uniform"``; ``"time_quadratic"``: uniform in sqrt(t).
    The end points are exactly ``T`` (default ``sde.T``) and ``eps``."""
    if isinstance(sde, sde_lib._ReverseSDE):
        sde = sde._fwd
    if not isinstance(sde, (sde_lib.subVPSDE, sde_lib.VPSDE, sde_lib.VESDE)):
        raise NotImplementedError(f"SDE class {sde.__class__.__name__} not yet supported.")
    steps, T, eps = int(steps), float(sde.T if T is None else T), float(eps)
    if steps < 1 or not 0.0 < eps < T:
        raise ValueError(f"dpm_time_grid: steps {steps} must be >= 1 and 0 < eps {eps} < T {T}")
    if skip_type == "logSNR":
        lam = np.linspace(_dpm_log_snr(sde, T), _dpm_log_snr(sde, eps), steps + 1)
        ts = _dpm_time_of_log_snr(sde, lam)
    elif skip_type == "time_uniform":
        ts = np.linspace(T, eps, steps + 1)
    elif skip_type == "time_quadratic":
        ts = np.linspace(np.sqrt(T), np.sqrt(eps), steps + 1) ** 2
    else:
        raise ValueError(f"unknown skip_type {skip_type!r}: expected one of {DPM_SKIP_TYPES}")
    ts = np.array(ts, dtype=np.float64)
    ts[0], ts[-1] = T, eps
    return ts


def dpm_coefficients(sde, times, order, lower_order_final=True, continuous=True):
    """dposer_dpm_coefficients: the (c_x, c_0, c_1) of every step x <- c_x x + c_0 D_i + c_1 D_{i-1} on the grid ``times`` (n + 1 decreasing
    times), float64 [n, 3].  Host only: no GPU is needed."""
    desc = sde_lib.sde_desc(sde, continuous)
    if desc is None:
        raise NotImplementedError(f"SDE class {sde.__class__.__name__} not yet supported.")
    times = np.ascontiguousarray(np.asarray(times, dtype=np.float64).reshape(-1))
    n = times.shape[0] - 1
    out = np.zeros((max(n, 1), 3), dtype=np.float64)
    _C.check(_C.lib().dposer_dpm_coefficients(C.byref(desc), times.ctypes.data_as(C.POINTER(C.c_double)), int(n), int(order),
                                              int(bool(lower_order_final)), out.ctypes.data_as(C.POINTER(C.c_double))), "dposer_dpm_coefficients")
    return out[:n]


def fused_dpm_supported(sde, model, continuous=True):
    """What ``dposer_dpm_sampler`` takes: a ScoreModelFC under the continuous sub-VP / VP / VE score function."""
    from .model import ScoreModelFC
    return bool(continuous) and isinstance(model, ScoreModelFC) and sde_lib.sde_desc(sde, True) is not None


def fused_dpm_sample(model, sde, x, times, *, order=2, lower_order_final=True, observation=None, mask=None, noise=None, seed=0,
                     traj_stride=0, continuous=True):
    """dposer_dpm_sampler: the ``len(times) - 1`` solver steps in ONE library call.  x [B, D] the state at times[0] (not modified); returns
    (trajs or None, x at times[-1], x0_hat = the last data prediction).  ``noise`` [n, B, D]: injected imputation draws (completion)."""
    from .model import ScoreModelFC
    if not isinstance(model, ScoreModelFC) or sde_lib.sde_desc(sde, continuous) is None:
        raise NotImplementedError("the DPM-Solver++ sampler runs a ScoreModelFC under sub-VP / VP / VE as one HIP call; there is no other path")
    times = torch.as_tensor(np.asarray(times, dtype=np.float64)).reshape(-1)
    n = int(times.shape[0]) - 1
    # the host entry's argument checks (grid, order, SDE kind) on the fp32 times the call will see, before any GPU work
    dpm_coefficients(sde, times.float().double().numpy(), order, lower_order_final, continuous)
    p = _fused_prelude(model, sde, x, times, max(n, 0), traj_stride, continuous, observation, mask, noise)
    x0_hat = torch.empty_like(p.x)
    if p.B == 0:
        return p.traj, p.x, x0_hat
    eng, B = p.eng, p.B
    hist = torch.empty_like(p.x)
    ws = eng.workspace(B, _C.WS_SHARED_T, max(n, 1), x.device)
    dpm = _C.DpmDesc(int(order), int(bool(lower_order_final)))
    _C.check(eng.lib.dposer_dpm_sampler(eng.h, _C.ptr(p.flat), _C.ptr(p.packed), _C.ptr(ws), C.byref(p.desc), C.byref(dpm), _C.ptr(p.x),
                                        _C.ptr(x0_hat), _C.ptr(hist), C.c_void_p(p.ts_host.data_ptr()), n, _C.ptr(p.obs), _C.ptr(p.msk),
                                        _C.ptr(p.nz), int(seed), _C.ptr(p.traj), int(traj_stride or 1),
                                        _C.ptr(eng.freq(x.device, model._fourier_W())), _C.ptr(model.sigmas), B, _C.stream_ptr()),
             "dposer_dpm_sampler")
    return p.traj, p.x, x0_hat


def get_dpm_sampler(sde, shape, inverse_scaler, steps=20, order=2, skip_type="logSNR", lower_order_final=True, continuous=True,
                    denoise=False, eps=1e-3, device="cuda"):
    """The few-step sampler: DPM-Solver++ (multistep, data prediction) of order 1 (= DDIM) or 2 on ``dpm_time_grid(sde, steps, skip_type,
    eps)``, ``steps`` network evaluations per sample in one library call (``fused_dpm_sample``).

    ``dpm_sampler(model, observation=None, mask=None, z=None, args=None, noise=None, seed=None, traj_stride=1)`` returns
    ``(trajs [steps // traj_stride, B, D], samples)`` shaped as ``pc_sampler`` returns them; ``denoise=True`` returns the last data
    prediction x0_hat in place of the state at ``eps``.  With ``observation`` and ``mask`` it completes: the state is imputed at every
    grid time before the network sees it, and the samples carry the observation on the mask.  A model or SDE the call does not
    take raises: there is no step-by-step path."""
    if isinstance(sde, sde_lib._ReverseSDE):
        sde = sde._fwd
    times = dpm_time_grid(sde, steps, skip_type, eps)
    call_count = [0]

    def dpm_sampler(model, observation=None, mask=None, z=None, args=None, noise=None, seed=None, traj_stride=1):
        if (observation is None) != (mask is None):
            raise ValueError("observation and mask go together")
        completion = observation is not None and (args is None or getattr(args, "task", "completion") in ["completion"])
        if z is not None and tuple(z.shape) != tuple(shape):
            raise ValueError(f"z {tuple(z.shape)} does not have the sampler's shape {tuple(shape)}")
        if completion and (tuple(observation.shape) != tuple(shape) or tuple(mask.shape) != tuple(shape)):
            raise ValueError(f"observation {tuple(observation.shape)} / mask {tuple(mask.shape)} do not have the sampler's shape {tuple(shape)}")
        if noise is not None and tuple(noise.shape) != (int(steps),) + tuple(shape):
            raise ValueError(f"noise {tuple(noise.shape)}: expected {(int(steps),) + tuple(shape)}")
        x = sde.prior_sampling(shape).to(device) if z is None else z
        call_count[0] += 1
        if seed is None:
            seed = (getattr(model, "_rng_seed", 0) * 7919 + call_count[0]) & 0xFFFFFFFFFFFF
        was_training = model.training
        model.eval()
        try:
            with torch.no_grad():
                trajs, x, x0_hat = fused_dpm_sample(model, sde, x, times, order=order, lower_order_final=lower_order_final,
                                                    observation=observation if completion else None, mask=mask if completion else None,
                                                    noise=noise if completion else None, seed=seed, traj_stride=traj_stride,
                                                    continuous=continuous)
        finally:
            model.train(was_training)
        if trajs is None:
            trajs = x.new_empty((0,) + tuple(x.shape))
        out = x0_hat if denoise else x
        if completion:
            out = observation * mask + out * (1 - mask)
        return trajs, out

    return dpm_sampler


GUIDED_METHODS = ("dps", "mcg")


def guided_noise_slots(method):
    """Slots per loop index of a guided sampler's ``noise`` [n_run, slots, B, D]: the predictor's z, then (MCG) the imputation draw."""
    return 2 if method == "mcg" else 1


def fused_guided_supported(sde, model, continuous):
    """What ``dposer_guided_sampler`` takes: a ScoreModelFC under the continuous sub-VP / VP score function."""
    from .model import ScoreModelFC
    return continuous and isinstance(sde, (sde_lib.subVPSDE, sde_lib.VPSDE)) and isinstance(model, ScoreModelFC) \
        and sde_lib.sde_desc(sde, continuous) is not None


def fused_guided_sample(model, sde, x, timesteps, observation, mask, *, method, grad_step=1.0, start_step=0, run_steps=-1, noise=None, seed=0,
                        traj_stride=0, continuous=True):
    """dposer_guided_sampler: loop indices [start_step, start_step + run_steps) (run_steps < 0: to N) of the MCG / DPS loop in ONE library
    call, then one 4-byte read of the non-finite flag.  x [B, D] initial state (consumed); returns (trajs or None, x, x_mean)."""
    N = int(sde.N)
    n_run = N - start_step if (run_steps < 0 or run_steps > N - start_step) else int(run_steps)
    _C.require_gpu(observation, "guided sampler observation")
    _C.require_gpu(mask, "guided sampler mask")
    p = _fused_prelude(model, sde, x, timesteps, n_run, traj_stride, continuous, observation, mask, noise, with_backward=True)   # (the dgrad reads the transposed copies)
    if p.B == 0:
        return p.traj, p.x, p.x_mean
    eng, B, packed = p.eng, p.B, p.packed
    ws = eng.workspace(B, _C.WS_GUIDED, max(n_run, 1), x.device)
    flag = torch.full((1,), 2 ** 31 - 1, dtype=torch.int32, device=x.device)
    _C.check(eng.lib.dposer_guided_sampler(eng.h, _C.ptr(p.flat), _C.ptr(packed), _C.ptr(ws), C.byref(p.desc), _C.ptr(p.x), _C.ptr(p.x_mean),
                                           C.c_void_p(p.ts_host.data_ptr()), int(start_step), int(run_steps), _C.ptr(p.obs), _C.ptr(p.msk),
                                           _C.ptr(p.nz), int(seed), _C.ptr(p.traj), int(traj_stride or 1), 1 if method == "mcg" else 0,
                                           float(grad_step), _C.ptr(flag), _C.ptr(eng.freq(x.device, model._fourier_W())), _C.ptr(model.sigmas), B,
                                           _C.stream_ptr()), "dposer_guided_sampler")
    bad = int(flag.item())                           # the call's one host read, after the loop
    if bad != 2 ** 31 - 1:
        raise ValueError("Consider reduce the value of parameter: grad_step={} (the gradient is not finite at loop index {})".format(grad_step, bad))
    return p.traj, p.x, p.x_mean


def get_guided_sampler(sde, shape, inverse_scaler, method, grad_step=1.0, continuous=True, denoise=True, eps=1e-3, device="cuda"):
    """The MCG and DPS completion samplers: the loop of sampling.py:455-461 over ``EulerMaruyamaPredictor.update_fn_guide`` (:191-207),
    for ``method == "mcg"`` followed by the imputation of :416-420 at every index; no imputation ahead of the step, no corrector.

    ``guided_sampler(model, observation, mask, z=None, start_step=0, *, traj_stride=1, noise=None, seed=None)`` returns
    ``(trajs [n, B, D], x_mean if denoise else x)`` like ``pc_sampler``; ``noise`` [n_run, 2 if mcg else 1, B, D] injects the draws
    (predictor z, imputation).  A ScoreModelFC under continuous sub-VP / VP on the GPU runs as ONE ``dposer_guided_sampler`` call;
    everything else steps ``update_fn_guide`` in Python."""
    method = str(method).lower()
    if method not in GUIDED_METHODS:
        raise ValueError(f"unknown guided sampler method {method!r}: expected one of {GUIDED_METHODS}")
    call_count = [0]

    def guided_sampler(model, observation, mask, z=None, start_step=0, *, traj_stride=1, noise=None, seed=None):
        if observation is None or mask is None:
            raise ValueError("the guided samplers need an observation and a mask")
        if tuple(observation.shape) != tuple(shape) or tuple(mask.shape) != tuple(shape):
            raise ValueError(f"observation {tuple(observation.shape)} / mask {tuple(mask.shape)} do not have the sampler's shape {tuple(shape)}")
        if z is not None and tuple(z.shape) != tuple(shape):
            raise ValueError(f"z {tuple(z.shape)} does not have the sampler's shape {tuple(shape)}")
        if not 0 <= start_step <= sde.N:
            raise ValueError(f"start_step {start_step} outside [0, {sde.N}]")
        n_run = sde.N - start_step
        slots = guided_noise_slots(method)
        if noise is not None and tuple(noise.shape) != (n_run, slots) + tuple(shape):
            raise ValueError(f"noise {tuple(noise.shape)}: expected {(n_run, slots) + tuple(shape)}")
        x = sde.prior_sampling(shape).to(device) if z is None else z
        if fused_guided_supported(sde, model, continuous):
            call_count[0] += 1
            if seed is None:
                seed = (model._rng_seed * 7919 + call_count[0]) & 0xFFFFFFFFFFFF
            was_training = model.training
            model.eval()
            try:
                with torch.no_grad():
                    trajs, x, x_mean = fused_guided_sample(model, sde, x, torch.linspace(sde.T, eps, sde.N), observation, mask, method=method,
                                                           grad_step=grad_step, start_step=start_step, noise=noise, seed=seed,
                                                           traj_stride=traj_stride, continuous=continuous)
            finally:
                model.train(was_training)
            if trajs is None:
                trajs = x.new_empty((0,) + tuple(x.shape))
            return trajs, (x_mean if denoise else x)
        # the reference semantics, step by step: update_fn_guide (its own autograd round trip and NaN check) + the imputation expression
        score_fn = mutils.get_score_fn(sde, model, train=False, continuous=continuous)
        pred = EulerMaruyamaPredictor(sde, score_fn, probability_flow=False)
        timesteps = torch.linspace(sde.T, eps, sde.N, device=x.device)
        trajs, x_mean = [], x
        real_randn_like = torch.randn_like
        for i in range(start_step, sde.N):
            vec_t = torch.ones(shape[0], device=x.device) * timesteps[i]
            nz = None if noise is None else noise[i - start_step]
            if nz is not None:                       # update_fn_guide draws its z itself: hand it this index's slot
                torch.randn_like = lambda t, _z=nz[0], **kw: _z
            try:
                x, x_mean = pred.update_fn_guide(x.detach(), vec_t, observation, mask, grad_step=grad_step)
            finally:
                torch.randn_like = real_randn_like
            x, x_mean = x.detach(), x_mean.detach()
            if method == "mcg":                      # sampling.py:416-420
                mean, std = sde.marginal_prob(observation, vec_t)
                x = x * (1 - mask) + (mean + (torch.randn_like(x) if nz is None else nz[1]) * std[:, None]) * mask
            if traj_stride and (i - start_step + 1) % traj_stride == 0:
                trajs.append(x)
        trajs = torch.stack(trajs, dim=0) if trajs else x.new_empty((0,) + tuple(x.shape))
        return trajs, (x_mean if denoise else x)

    return guided_sampler


JOINT_GUIDED_NORMS = ("batch", "sample")


def fused_joint_guided_supported(sde, model, continuous):
    """What ``dposer_joint_guided_sampler`` takes: ``fused_guided_supported`` and a network on 21 axis-angle joints (63 inputs)."""
    return bool(fused_guided_supported(sde, model, continuous)) and int(model.n_poses) * int(model.joint_dim) == 63


def _joint_guided_problem(body_model, normalizer, joints3d, joints_conf, obs_joints, root_orient, trans, betas, B):
    """Host checks of a 3D-joint observation for ``B`` poses (shapes, ``obs_joints`` range and distinctness -- before any device work),
    then its device tensors: (obs [B, n_obs, 3], conf [B, n_obs] or None, rows list or None)."""
    from ...tasks.motion_denoising import _partial_observation
    if joints3d.dim() != 3 or tuple(joints3d.shape[::2]) != (B, 3) or not 1 <= joints3d.shape[1] <= 22:
        raise ValueError(f"joints3d must be [{B}, 1..22, 3], got {list(joints3d.shape)}")
    for name, t in (("root_orient", root_orient), ("trans", trans)):
        if t is not None and tuple(t.shape) != (B, 3):
            raise ValueError(f"{name} must be [{B}, 3], got {list(t.shape)}")
    if betas is not None and (betas.dim() != 2 or betas.shape[0] != B):
        raise ValueError(f"betas must be [{B}, n], got {list(betas.shape)}")
    conf, rows = _partial_observation(joints3d, joints_conf, obs_joints, 22)
    return joints3d, conf, rows


def fused_joint_guided_sample(model, sde, x, timesteps, body_model, normalizer, joints3d, *, joints_conf=None, obs_rows=None, root_orient=None,
                              trans=None, betas=None, norm="sample", grad_step=1.0, start_step=0, run_steps=-1, noise=None, seed=0, traj_stride=0,
                              continuous=True):
    """dposer_joint_guided_sampler: loop indices [start_step, start_step + run_steps) (run_steps < 0: to N) of DPS on observed 3D joints in
    ONE library call, then one 4-byte read of the non-finite flag.  x [B, 63] initial state (consumed); ``joints3d`` [B, n_obs, 3],
    ``joints_conf`` [B, n_obs] or None, ``obs_rows`` a list of n_obs distinct joints in [0, 22) or None -- already checked
    (``get_joint_guided_sampler`` does).  Returns (trajs or None, x, x_mean)."""
    from ...tasks._fused import normalizer_tables
    N = int(sde.N)
    n_run = N - start_step if (run_steps < 0 or run_steps > N - start_step) else int(run_steps)
    _C.require_gpu(joints3d, "joint-guided sampler observation")
    p = _fused_prelude(model, sde, x, timesteps, n_run, traj_stride, continuous, None, None, noise, with_backward=True)
    if p.B == 0:
        return p.traj, p.x, p.x_mean
    eng, B, dev = p.eng, p.B, x.device
    core = body_model.bm
    with torch.no_grad():
        _, j_rest, batched = core.rest_shape(betas, None)
    f32 = lambda t: None if t is None else t.detach().to(dev).contiguous().float()
    obs, conf, root, tr, jr = f32(joints3d), f32(joints_conf), f32(root_orient), f32(trans), f32(j_rest)
    mode, na, nb = normalizer_tables(normalizer, p.x)
    rows_d = None if obs_rows is None else torch.tensor([int(r) for r in obs_rows], dtype=torch.int32, device=dev)
    ws = eng.workspace(B, _C.WS_GUIDED, max(n_run, 1), dev)
    scratch = torch.empty(eng.lib.dposer_joint_guided_scratch_bytes(B), dtype=torch.uint8, device=dev)
    flag = torch.full((1,), 2 ** 31 - 1, dtype=torch.int32, device=dev)
    _C.check(eng.lib.dposer_joint_guided_sampler(eng.h, _C.ptr(p.flat), _C.ptr(p.packed), _C.ptr(ws), C.byref(p.desc), _C.ptr(p.x), _C.ptr(p.x_mean),
                                                 C.c_void_p(p.ts_host.data_ptr()), int(start_step), int(run_steps), core._handle(), mode, _C.ptr(na),
                                                 _C.ptr(nb), _C.ptr(root), _C.ptr(tr), _C.ptr(jr), 1 if batched else 0, _C.ptr(obs), _C.ptr(conf),
                                                 _C.ptr(rows_d), int(obs.shape[1]), JOINT_GUIDED_NORMS.index(norm), _C.ptr(p.nz), int(seed),
                                                 _C.ptr(p.traj), int(traj_stride or 1), float(grad_step), _C.ptr(flag), _C.ptr(scratch),
                                                 _C.ptr(eng.freq(dev, model._fourier_W())), _C.ptr(model.sigmas), B, _C.stream_ptr()),
             "dposer_joint_guided_sampler")
    bad = int(flag.item())                           # the call's one host read, after the loop
    if bad != 2 ** 31 - 1:
        raise ValueError("Consider reduce the value of parameter: grad_step={} (the gradient is not finite at loop index {})".format(grad_step, bad))
    return p.traj, p.x, p.x_mean


def joint_guided_step(rsde, body_model, normalizer, x_t, t, z, obs, conf, rows, root_orient, trans, betas, norm, grad_step):
    """One step of DPS on observed 3D joints with torch autograd through the score function and ``fk_joints(grad="chain")`` -- what
    ``dposer_joint_guided_sampler`` runs per loop index, for the models and SDEs it does not take.  Returns (y_hat, y_mean)."""
    import contextlib
    x_t = x_t.detach().requires_grad_()
    dt = -1.0 / rsde.N
    model = getattr(getattr(rsde, "_score_fn", None), "model", None)
    only_x = model.input_grad_only() if hasattr(model, "input_grad_only") else contextlib.nullcontext()
    with torch.enable_grad():
        with only_x:
            drift, diffusion, alpha, sigma_2, score = rsde.sde(x_t, t, None, None, guide=True)
        y_mean = x_t.detach() + drift.detach() * dt
        y_hat = y_mean + diffusion[:, None] * np.sqrt(-dt) * z
        y0 = (x_t + sigma_2[:, None] * score) / alpha
        joints = body_model.fk_joints(normalizer.offline_denormalize(y0), root_orient=root_orient, trans=trans, betas=betas, grad="chain")
        idx = torch.arange(obs.shape[1], device=obs.device) if rows is None else torch.tensor(rows, dtype=torch.long, device=obs.device)
        c = torch.ones(obs.shape[:2], dtype=y0.dtype, device=obs.device) if conf is None else conf
        live = c > 0                                 # false for 0, negatives and NaN; a dead entry never enters a sum
        r = joints[:, idx] - torch.where(live[..., None], obs, torch.zeros_like(obs))
        s = (torch.where(live, c, torch.zeros_like(c)) * (r * r).sum(dim=2)).sum(dim=1)
        if norm == "batch":
            s = s.sum().reshape(1)
        on = s > 0                                   # norm == 0: no guidance (sqrt has no gradient there)
        total = torch.where(on, torch.sqrt(torch.where(on, s, torch.ones_like(s))), torch.zeros_like(s)).sum()
        g = torch.autograd.grad(total, x_t)[0] if total.requires_grad else torch.zeros_like(y_hat)
    if not torch.isfinite(g).all() or not torch.isfinite(s).all():
        raise ValueError("Consider reduce the value of parameter: grad_step={}".format(grad_step))
    return (y_hat - grad_step * g).detach(), y_mean.detach()


def get_joint_guided_sampler(sde, shape, body_model, normalizer, grad_step=1.0, norm="sample", continuous=True, denoise=True, eps=1e-3,
                             device="cuda"):
    """DPS on observed 3D joints: the loop of ``get_guided_sampler`` with the posed body joints as the measurement -- a head and two wrists
    from a headset, a detector's joints with an occluded limb -- instead of a pose-space mask; several calls (or a tiled batch) draw
    several plausible bodies for one observation.

    ``sampler(model, joints3d, joints_conf=None, obs_joints=None, root_orient=None, trans=None, betas=None, z=None, start_step=0, *,
    traj_stride=1, noise=None, seed=None)`` returns ``(trajs [n, B, 63], x_mean if denoise else x)`` in the network's normalised space.
    ``joints3d`` [B, n_obs, 3]; ``joints_conf`` [B, n_obs] or [n_obs]: an entry counts iff its confidence is > 0 and what lies under a dead
    entry may be NaN; ``obs_joints``: the n_obs distinct joints in [0, 22) the columns observe (default 0 .. n_obs - 1).  ``norm``:
    "sample" -- every row is its own problem, guided by the gradient of its own residual norm -- or "batch", the reference's
    ``torch.norm`` over the whole batch.  A row (or, under "batch", a batch) without a live entry is sampled unconditionally.  ``noise``
    [n_run, 1, B, 63] injects the draws.  A ScoreModelFC on 63 inputs under continuous sub-VP / VP runs as ONE
    ``dposer_joint_guided_sampler`` call; everything else steps ``joint_guided_step`` in Python."""
    if norm not in JOINT_GUIDED_NORMS:
        raise ValueError(f"unknown norm scope {norm!r}: expected one of {JOINT_GUIDED_NORMS}")
    if len(shape) != 2 or int(shape[1]) != 63:
        raise ValueError(f"the joint-guided sampler works on [B, 63] axis-angle body poses, got shape {tuple(shape)}")
    call_count = [0]

    def joint_guided_sampler(model, joints3d, joints_conf=None, obs_joints=None, root_orient=None, trans=None, betas=None, z=None, start_step=0, *,
                             traj_stride=1, noise=None, seed=None):
        B = int(shape[0])
        obs, conf, rows = _joint_guided_problem(body_model, normalizer, joints3d, joints_conf, obs_joints, root_orient, trans, betas, B)
        if z is not None and tuple(z.shape) != tuple(shape):
            raise ValueError(f"z {tuple(z.shape)} does not have the sampler's shape {tuple(shape)}")
        if not 0 <= start_step <= sde.N:
            raise ValueError(f"start_step {start_step} outside [0, {sde.N}]")
        n_run = sde.N - start_step
        if noise is not None and tuple(noise.shape) != (n_run, 1) + tuple(shape):
            raise ValueError(f"noise {tuple(noise.shape)}: expected {(n_run, 1) + tuple(shape)}")
        x = sde.prior_sampling(shape).to(device) if z is None else z
        _C.require_gpu(x, "sampler state")
        _C.require_gpu(joints3d, "joint-guided sampler observation")
        if fused_joint_guided_supported(sde, model, continuous):
            call_count[0] += 1
            if seed is None:
                seed = (model._rng_seed * 7919 + call_count[0]) & 0xFFFFFFFFFFFF
            was_training = model.training
            model.eval()
            try:
                with torch.no_grad():
                    trajs, x, x_mean = fused_joint_guided_sample(model, sde, x, torch.linspace(sde.T, eps, sde.N), body_model, normalizer, obs,
                                                                 joints_conf=conf, obs_rows=rows, root_orient=root_orient, trans=trans, betas=betas,
                                                                 norm=norm, grad_step=grad_step, start_step=start_step, noise=noise, seed=seed,
                                                                 traj_stride=traj_stride, continuous=continuous)
            finally:
                model.train(was_training)
            if trajs is None:
                trajs = x.new_empty((0,) + tuple(x.shape))
            return trajs, (x_mean if denoise else x)
        score_fn = mutils.get_score_fn(sde, model, train=False, continuous=continuous)
        rsde = sde.reverse(score_fn, False)
        timesteps = torch.linspace(sde.T, eps, sde.N, device=x.device)
        obs_d = obs.to(x.device).float()
        conf_d = None if conf is None else conf.to(x.device).float()
        trajs, x_mean = [], x
        for i in range(start_step, sde.N):
            vec_t = torch.ones(shape[0], device=x.device) * timesteps[i]
            zi = torch.randn_like(x) if noise is None else noise[i - start_step, 0]
            x, x_mean = joint_guided_step(rsde, body_model, normalizer, x, vec_t, zi, obs_d, conf_d, rows, root_orient, trans, betas, norm, grad_step)
            if traj_stride and (i - start_step + 1) % traj_stride == 0:
                trajs.append(x)
        trajs = torch.stack(trajs, dim=0) if trajs else x.new_empty((0,) + tuple(x.shape))
        return trajs, (x_mean if denoise else x)

    return joint_guided_sampler


def _keypoint_guided_problem(keypoints2d, keypoints_conf, obs_joints, cam_t, camera_center, focal_length, sigma, z_near, root_orient, betas, B):
    """Host checks of a 2D-keypoint observation for ``B`` poses and its camera (shapes, ``obs_joints`` range and distinctness, the scalars --
    before any device work): (keypoints [B, n_obs, 2], conf [B, n_obs] or None, rows list or None, focal [B] float32 on the keypoints'
    device).  ``focal_length``: a number, or a tensor of 1 or B values."""
    from ...tasks.motion_denoising import _partial_observation
    if keypoints2d.dim() != 3 or tuple(keypoints2d.shape[::2]) != (B, 2) or not 1 <= keypoints2d.shape[1] <= 22:
        raise ValueError(f"keypoints2d must be [{B}, 1..22, 2], got {list(keypoints2d.shape)}")
    if cam_t is None or camera_center is None:
        raise ValueError("cam_t [B, 3] and camera_center [B, 2] are required")
    for name, t, n in (("cam_t", cam_t, 3), ("camera_center", camera_center, 2), ("root_orient", root_orient, 3)):
        if t is not None and tuple(t.shape) != (B, n):
            raise ValueError(f"{name} must be [{B}, {n}], got {list(t.shape)}")
    if betas is not None and (betas.dim() != 2 or betas.shape[0] != B):
        raise ValueError(f"betas must be [{B}, n], got {list(betas.shape)}")
    if not float(z_near) > 0 or not np.isfinite(float(z_near)):
        raise ValueError(f"z_near must be positive and finite, got {z_near}")
    if not (float(sigma) <= 0 or 1e-18 <= float(sigma) <= 1e18):
        raise ValueError(f"sigma must be <= 0 (no robustifier) or in [1e-18, 1e18], got {sigma}")
    focal = torch.as_tensor(focal_length, dtype=torch.float32).reshape(-1)
    if focal.numel() not in (1, B):
        raise ValueError(f"focal_length must be a number or [{B}], got {list(focal.shape)}")
    focal = focal.expand(B).contiguous().to(keypoints2d.device)
    try:
        conf, rows = _partial_observation(keypoints2d, keypoints_conf, obs_joints, 22)
    except ValueError as e:                          # the shared rule's messages, in this function's argument names
        raise ValueError(str(e).replace("joints3d", "keypoints2d").replace("joints_conf", "keypoints_conf")) from None
    return keypoints2d, conf, rows, focal


def fused_keypoint_guided_sample(model, sde, x, timesteps, body_model, normalizer, keypoints2d, *, keypoints_conf=None, obs_rows=None, cam_t,
                                 camera_center, focal, sigma=100.0, z_near=0.1, root_orient=None, betas=None, norm="sample", grad_step=1.0,
                                 start_step=0, run_steps=-1, noise=None, seed=0, traj_stride=0, continuous=True):
    """dposer_keypoint_guided_sampler: loop indices [start_step, start_step + run_steps) (run_steps < 0: to N) of DPS on observed 2D
    keypoints in ONE library call, then one 4-byte read of the non-finite flag.  x [B, 63] initial state (consumed); ``keypoints2d``
    [B, n_obs, 2] pixels, ``keypoints_conf`` [B, n_obs] or None, ``obs_rows`` a list of n_obs distinct joints in [0, 22) or None, ``cam_t``
    [B, 3], ``camera_center`` [B, 2], ``focal`` [B] -- already checked (``get_keypoint_guided_sampler`` does).  Returns (trajs or None, x, x_mean)."""
    from ...tasks._fused import normalizer_tables
    N = int(sde.N)
    n_run = N - start_step if (run_steps < 0 or run_steps > N - start_step) else int(run_steps)
    _C.require_gpu(keypoints2d, "keypoint-guided sampler observation")
    p = _fused_prelude(model, sde, x, timesteps, n_run, traj_stride, continuous, None, None, noise, with_backward=True)
    if p.B == 0:
        return p.traj, p.x, p.x_mean
    eng, B, dev = p.eng, p.B, x.device
    core = body_model.bm
    with torch.no_grad():
        _, j_rest, batched = core.rest_shape(betas, None)
    f32 = lambda t: None if t is None else t.detach().to(dev).contiguous().float()
    kp, conf, root, tr, jr, fo, ce = f32(keypoints2d), f32(keypoints_conf), f32(root_orient), f32(cam_t), f32(j_rest), f32(focal), f32(camera_center)
    mode, na, nb = normalizer_tables(normalizer, p.x)
    rows_d = None if obs_rows is None else torch.tensor([int(r) for r in obs_rows], dtype=torch.int32, device=dev)
    ws = eng.workspace(B, _C.WS_GUIDED, max(n_run, 1), dev)
    scratch = torch.empty(eng.lib.dposer_keypoint_guided_scratch_bytes(B), dtype=torch.uint8, device=dev)
    flag = torch.full((1,), 2 ** 31 - 1, dtype=torch.int32, device=dev)
    _C.check(eng.lib.dposer_keypoint_guided_sampler(eng.h, _C.ptr(p.flat), _C.ptr(p.packed), _C.ptr(ws), C.byref(p.desc), _C.ptr(p.x), _C.ptr(p.x_mean),
                                                    C.c_void_p(p.ts_host.data_ptr()), int(start_step), int(run_steps), core._handle(), mode, _C.ptr(na),
                                                    _C.ptr(nb), _C.ptr(root), _C.ptr(tr), _C.ptr(jr), 1 if batched else 0, _C.ptr(kp), _C.ptr(conf),
                                                    _C.ptr(rows_d), int(kp.shape[1]), _C.ptr(fo), _C.ptr(ce), float(sigma), float(z_near),
                                                    JOINT_GUIDED_NORMS.index(norm), _C.ptr(p.nz), int(seed), _C.ptr(p.traj), int(traj_stride or 1),
                                                    float(grad_step), _C.ptr(flag), _C.ptr(scratch), _C.ptr(eng.freq(dev, model._fourier_W())),
                                                    _C.ptr(model.sigmas), B, _C.stream_ptr()),
             "dposer_keypoint_guided_sampler")
    bad = int(flag.item())                           # the call's one host read, after the loop
    if bad != 2 ** 31 - 1:
        raise ValueError("Consider reduce the value of parameter: grad_step={} (the gradient is not finite at loop index {})".format(grad_step, bad))
    return p.traj, p.x, p.x_mean


def keypoint_residual_sum(joints, keypoints, conf, rows, focal, center, sigma, z_near):
    """s [B] of the keypoint-residual stage on posed joints ``joints`` [B, >= 22, 3] in torch, differentiable in ``joints`` -- the rule of
    ``dposer_keypoint_guide_stage`` (include/dposer_hip.h): live iff c > 0 and Z > z_near, r = focal J_xy / Z - (k - centre),
    s = sum_live c^2 (rho(ru) + rho(rv)) with rho = gmof (sigma <= 0: r^2).  Returns (s, live [B, n_obs])."""
    idx = torch.arange(keypoints.shape[1], device=keypoints.device) if rows is None else torch.tensor(rows, dtype=torch.long, device=keypoints.device)
    c = torch.ones(keypoints.shape[:2], dtype=joints.dtype, device=keypoints.device) if conf is None else conf
    P = joints[:, idx]
    Z = P[..., 2]
    live = (c > 0) & (Z > z_near)                    # false for 0, negatives and NaN; a dead entry never enters a sum
    Zs = torch.where(live, Z, torch.ones_like(Z))
    k = torch.where(live[..., None], keypoints, torch.zeros_like(keypoints))
    r = focal[:, None, None] * (P[..., :2] / Zs[..., None]) - (k - center[:, None, :])
    r2 = r * r
    rho = (sigma ** 2 * r2) / (sigma ** 2 + r2) if sigma > 0 else r2
    c = torch.where(live, c, torch.zeros_like(c))
    return (c * c * torch.where(live[..., None], rho, torch.zeros_like(rho)).sum(dim=2)).sum(dim=1), live


def keypoint_guided_step(rsde, body_model, normalizer, x_t, t, z, kp, conf, rows, cam_t, center, focal, sigma, z_near, root_orient, betas, norm,
                         grad_step):
    """One step of DPS on observed 2D keypoints with torch autograd through the score function and ``fk_joints(grad="chain")`` -- what
    ``dposer_keypoint_guided_sampler`` runs per loop index, for the models and SDEs it does not take.  Returns (y_hat, y_mean)."""
    import contextlib
    x_t = x_t.detach().requires_grad_()
    dt = -1.0 / rsde.N
    model = getattr(getattr(rsde, "_score_fn", None), "model", None)
    only_x = model.input_grad_only() if hasattr(model, "input_grad_only") else contextlib.nullcontext()
    with torch.enable_grad():
        with only_x:
            drift, diffusion, alpha, sigma_2, score = rsde.sde(x_t, t, None, None, guide=True)
        y_mean = x_t.detach() + drift.detach() * dt
        y_hat = y_mean + diffusion[:, None] * np.sqrt(-dt) * z
        y0 = (x_t + sigma_2[:, None] * score) / alpha
        joints = body_model.fk_joints(normalizer.offline_denormalize(y0), root_orient=root_orient, trans=cam_t, betas=betas, grad="chain")
        s, _ = keypoint_residual_sum(joints, kp, conf, rows, focal, center, sigma, z_near)
        if norm == "batch":
            s = s.sum().reshape(1)
        on = s > 0                                   # norm == 0: no guidance (sqrt has no gradient there)
        total = torch.where(on, torch.sqrt(torch.where(on, s, torch.ones_like(s))), torch.zeros_like(s)).sum()
        g = torch.autograd.grad(total, x_t)[0] if total.requires_grad else torch.zeros_like(y_hat)
    if not torch.isfinite(g).all() or not torch.isfinite(s).all():
        raise ValueError("Consider reduce the value of parameter: grad_step={}".format(grad_step))
    return (y_hat - grad_step * g).detach(), y_mean.detach()


def get_keypoint_guided_sampler(sde, shape, body_model, normalizer, focal_length=5000.0, sigma=100.0, z_near=0.1, grad_step=1.0, norm="sample",
                                continuous=True, denoise=True, eps=1e-3, device="cuda"):
    """DPS on observed 2D keypoints: the loop of ``get_joint_guided_sampler`` with a pinhole camera and SMPLify's robust reprojection
    residual as the measurement -- a detector's keypoints.  Several calls (or a tiled batch) draw several bodies that reproject onto the
    same keypoints and differ in what one view does not fix, depth above all.

    ``sampler(model, keypoints2d, keypoints_conf=None, obs_joints=None, *, cam_t, camera_center, root_orient=None, betas=None, z=None,
    start_step=0, traj_stride=1, noise=None, seed=None)`` returns ``(trajs [n, B, 63], x_mean if denoise else x)`` in the network's
    normalised space.  ``keypoints2d`` [B, n_obs, 2] pixels; ``keypoints_conf`` [B, n_obs] or [n_obs]; ``obs_joints``: the n_obs distinct
    tree joints in [0, 22) the columns observe (default 0 .. n_obs - 1; the vertex-selected extra joints of the 49-joint map are not
    supported); ``cam_t`` [B, 3] the camera translation, added to the posed joints as SMPLify's ``transl=camera_t``; ``camera_center``
    [B, 2]; ``focal_length`` a number or [B].  An entry counts iff its confidence is > 0 AND its joint lies in front of ``z_near`` (metres)
    at that evaluation; what lies under a dead entry may be NaN.  The residual is ``focal X / Z - (k - centre)`` under the Geman-McClure
    ``sigma`` (<= 0: none), weighted by the squared confidence.  ``norm``, ``noise``, ``seed``: as in ``get_joint_guided_sampler``.  A
    ScoreModelFC on 63 inputs under continuous sub-VP / VP runs as ONE ``dposer_keypoint_guided_sampler`` call; everything else steps
    ``keypoint_guided_step`` in Python."""
    if norm not in JOINT_GUIDED_NORMS:
        raise ValueError(f"unknown norm scope {norm!r}: expected one of {JOINT_GUIDED_NORMS}")
    if len(shape) != 2 or int(shape[1]) != 63:
        raise ValueError(f"the keypoint-guided sampler works on [B, 63] axis-angle body poses, got shape {tuple(shape)}")
    if not float(z_near) > 0 or not np.isfinite(float(z_near)):
        raise ValueError(f"z_near must be positive and finite, got {z_near}")
    call_count = [0]

    def keypoint_guided_sampler(model, keypoints2d, keypoints_conf=None, obs_joints=None, *, cam_t, camera_center, root_orient=None, betas=None, z=None,
                                start_step=0, traj_stride=1, noise=None, seed=None):
        B = int(shape[0])
        kp, conf, rows, focal = _keypoint_guided_problem(keypoints2d, keypoints_conf, obs_joints, cam_t, camera_center, focal_length, sigma, z_near,
                                                         root_orient, betas, B)
        if z is not None and tuple(z.shape) != tuple(shape):
            raise ValueError(f"z {tuple(z.shape)} does not have the sampler's shape {tuple(shape)}")
        if not 0 <= start_step <= sde.N:
            raise ValueError(f"start_step {start_step} outside [0, {sde.N}]")
        n_run = sde.N - start_step
        if noise is not None and tuple(noise.shape) != (n_run, 1) + tuple(shape):
            raise ValueError(f"noise {tuple(noise.shape)}: expected {(n_run, 1) + tuple(shape)}")
        x = sde.prior_sampling(shape).to(device) if z is None else z
        _C.require_gpu(x, "sampler state")
        _C.require_gpu(keypoints2d, "keypoint-guided sampler observation")
        if fused_joint_guided_supported(sde, model, continuous):
            call_count[0] += 1
            if seed is None:
                seed = (model._rng_seed * 7919 + call_count[0]) & 0xFFFFFFFFFFFF
            was_training = model.training
            model.eval()
            try:
                with torch.no_grad():
                    trajs, x, x_mean = fused_keypoint_guided_sample(model, sde, x, torch.linspace(sde.T, eps, sde.N), body_model, normalizer, kp,
                                                                    keypoints_conf=conf, obs_rows=rows, cam_t=cam_t, camera_center=camera_center,
                                                                    focal=focal, sigma=sigma, z_near=z_near, root_orient=root_orient, betas=betas,
                                                                    norm=norm, grad_step=grad_step, start_step=start_step, noise=noise, seed=seed,
                                                                    traj_stride=traj_stride, continuous=continuous)
            finally:
                model.train(was_training)
            if trajs is None:
                trajs = x.new_empty((0,) + tuple(x.shape))
            return trajs, (x_mean if denoise else x)
        score_fn = mutils.get_score_fn(sde, model, train=False, continuous=continuous)
        rsde = sde.reverse(score_fn, False)
        timesteps = torch.linspace(sde.T, eps, sde.N, device=x.device)
        f32 = lambda t: None if t is None else t.to(x.device).float()
        kp_d, conf_d, cam_d, cen_d, foc_d, root_d, betas_d = f32(kp), f32(conf), f32(cam_t), f32(camera_center), f32(focal), f32(root_orient), f32(betas)
        trajs, x_mean = [], x
        for i in range(start_step, sde.N):
            vec_t = torch.ones(shape[0], device=x.device) * timesteps[i]
            zi = torch.randn_like(x) if noise is None else noise[i - start_step, 0]
            x, x_mean = keypoint_guided_step(rsde, body_model, normalizer, x, vec_t, zi, kp_d, conf_d, rows, cam_d, cen_d, foc_d, float(sigma),
                                             float(z_near), root_d, betas_d, norm, grad_step)
            if traj_stride and (i - start_step + 1) % traj_stride == 0:
                trajs.append(x)
        trajs = torch.stack(trajs, dim=0) if trajs else x.new_empty((0,) + tuple(x.shape))
        return trajs, (x_mean if denoise else x)

    return keypoint_guided_sampler


def get_ode_sampler(sde, shape, inverse_scaler, denoise=False, rtol=1e-5, atol=1e-5, method="RK45", eps=1e-3, device="cuda", driver=None,
                    n_steps=None):
    """Probability-flow ODE sampler (sampling.py:471-542): ``ode_sampler(model, z=None) -> (nfe, samples)``.

    The adaptive RK45 steps follow scipy's controller exactly like the reference (tolerances and ``nfe`` are part of the
    result); with ``driver='device'`` (default for RK45, ``likelihood.get_likelihood_fn`` has the details) the state never leaves
    the GPU, with ``driver='scipy'`` ``scipy.integrate.solve_ivp`` drives it from the host.  Each drift evaluation is one HIP
    forward of the score network.  ``denoise`` adds one noise-free reverse-diffusion predictor step at ``eps`` (:492-499)."""
    import os
    from .likelihood import FusedPfRhs, probability_flow_drift
    from scipy import integrate
    fixed = method in ("rk4", "euler")      # fixed-step, fully asynchronous device integration (likelihood.get_likelihood_fn has the details)
    if fixed and not n_steps:
        raise ValueError(f"method={method!r} is a fixed-step integrator: pass n_steps")
    driver = driver or os.environ.get("DPOSER_ODE_DRIVER") or ("device" if (method == "RK45" or fixed) else "scipy")
    if driver == "device" and not (method == "RK45" or fixed):
        raise NotImplementedError("the device-resident driver implements RK45 (the reference's default), rk4 and euler; use driver='scipy'")
    if fixed and driver != "device":
        raise NotImplementedError("fixed-step methods run on the device-resident driver")

    def ode_sampler(model, z=None):
        with torch.no_grad():
            x = sde.prior_sampling(shape).to(device) if z is None else z

            def rhs_generic(t, state):
                xt = state.reshape(shape).float()
                vec_t = torch.full((shape[0],), float(t), device=device, dtype=torch.float32)
                return probability_flow_drift(sde, model, xt, vec_t).reshape(-1).double()

            rhs_dev = FusedPfRhs.build(sde, model, tuple(x.shape), x.device) or rhs_generic      # three launches around the forward

            if driver == "device":
                from .ode_device import solve_fixed, solve_rk45
                if fixed:
                    end, nfev = solve_fixed(rhs_dev, sde.T, eps, x.reshape(-1).double(), int(n_steps), method=method)
                else:
                    end, nfev = solve_rk45(rhs_dev, sde.T, eps, x.reshape(-1).double(), rtol=rtol, atol=atol)
                x = end.reshape(shape).float()
            else:
                sol = integrate.solve_ivp(lambda t, s_: rhs_dev(t, torch.from_numpy(s_).to(device)).cpu().numpy(), (sde.T, eps),
                                          mutils.to_flattened_numpy(x), rtol=rtol, atol=atol, method=method)
                nfev = sol.nfev
                x = torch.from_numpy(sol.y[:, -1].reshape(shape)).to(device, torch.float32)
            if denoise:
                score_fn = get_score_fn(sde, model, train=False, continuous=True)
                vec_eps = torch.full((shape[0],), float(eps), device=device, dtype=torch.float32)
                x = ReverseDiffusionPredictor(sde, score_fn, probability_flow=False).update_fn(x, vec_eps)[1]
            return nfev, inverse_scaler(x)

    return ode_sampler
