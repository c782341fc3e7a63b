"""Test infrastructure for the one-call predictor-corrector sampler (dposer_pc_sampler).

(a) ``pc_loop``: the loop of sampling.py:455-461 for every registered predictor x corrector, on the CPU oracle
    (``oracle.score_ref.score_fn`` / ``impute``, in the manner of tests/pf_ref.py): ReverseDiffusion (sampling.py:215-220 over
    RSDE.discretize sde_lib.py:111-117 and the SDE's own discretize :52-69 / :167-175 / :279-287), AncestralSampling (:233-253),
    None (:262-270), Euler-Maruyama (``score_ref.em_step``); Langevin (``score_ref.langevin_step``), ALD (:319-339).  The draws come
    from ``draw()`` in the reference's order -- a draw is made exactly where the reference calls torch.randn_like -- and are also laid
    out in the slots of the library's ``noise`` argument (a slot the reference does not draw for stays zero).

(b) the three predictor stages and the ALD stage on ``sde_ref.E`` pairs: the float64 value and the first-order fp32 band, every
    operation counted as sde_ref counts them.  Table entries enter as exact fp32 numbers; the VE branch at timestep 0 (adjacent sigma 0,
    ancestral std exactly 0) is an exact value with zero bound, not a square root at 0.  The keyword faults (``pf_factor``,
    ``adj_shift``, ``drop_alpha``, ``linear_sqrt``) seed the mutation checks of tests/test_pc_sampler_cpu.py.
"""
import numpy as np
import torch

import sde_ref as S
from oracle import score_ref as R

F32 = np.float32
PREDICTORS = ("none", "euler_maruyama", "reverse_diffusion", "ancestral_sampling")
CORRECTORS = ("none", "langevin", "ald")


# ---- (a) the loop on the CPU oracle --------------------------------------------------------------------------------------------------
def discrete_table(sde, dtype=torch.float32):
    """discrete_betas (sub-VP / VP, sde_lib.py:136, 197) or discrete_sigmas (VE, :247) of an oracle SDE, as torch builds them."""
    if sde.name == "VESDE":
        return torch.exp(torch.linspace(np.log(sde.smin), np.log(sde.smax), sde.N)).to(dtype)
    return sde.discrete_betas.to(dtype)


def _timestep(sde, t):
    return (t * (sde.N - 1) / sde.T).long()


def _discretize(sde, table, x, t):
    """The forward SDE's discretize: base Euler form (sub-VP), DDPM (VP), SMLD (VE)."""
    if sde.name == "VPSDE":
        beta = table[_timestep(sde, t)]
        alpha = 1.0 - beta
        return torch.sqrt(alpha)[:, None] * x - x, torch.sqrt(beta)
    if sde.name == "VESDE":
        ts = _timestep(sde, t)
        sigma = table[ts]
        adj = torch.where(ts == 0, torch.zeros_like(t), table[ts - 1])
        return torch.zeros_like(x), torch.sqrt(sigma ** 2 - adj ** 2)
    dt = 1 / sde.N
    drift, diffusion = sde.sde(x, t)
    return drift * dt, diffusion * torch.sqrt(torch.tensor(dt, dtype=x.dtype))


def reverse_diffusion_step(p, sde, table, x, t, z, probability_flow=False, **fw):
    f, G = _discretize(sde, table, x, t)
    rev_f = f - G[:, None] ** 2 * R.score_fn(p, sde, x, t, **fw)          # full score term also under probability flow (sde_lib.py:114-115)
    rev_G = torch.zeros_like(G) if probability_flow else G
    x_mean = x - rev_f
    return x_mean + rev_G[:, None] * z, x_mean


def ancestral_step(p, sde, table, x, t, z, **fw):
    ts = _timestep(sde, t)
    score = R.score_fn(p, sde, x, t, **fw)
    if sde.name == "VESDE":
        sigma = table[ts]
        adj = torch.where(ts == 0, torch.zeros_like(t), table[ts - 1])
        x_mean = x + score * (sigma ** 2 - adj ** 2)[:, None]
        std = torch.sqrt((adj ** 2 * (sigma ** 2 - adj ** 2)) / (sigma ** 2))
        return x_mean + std[:, None] * z, x_mean
    assert sde.name == "VPSDE", "ancestral sampling: VE / VP only"
    beta = table[ts]
    x_mean = (x + beta[:, None] * score) / torch.sqrt(1.0 - beta)[:, None]
    return x_mean + torch.sqrt(beta)[:, None] * z, x_mean


def ald_step(p, sde, table, x, t, noise, snr, **fw):
    alpha = torch.ones_like(t) if sde.name == "VESDE" else (1.0 - table)[_timestep(sde, t)]
    std = sde.marginal_prob(x, t)[1]
    grad = R.score_fn(p, sde, x, t, **fw)
    step = (snr * std) ** 2 * 2 * alpha
    x_mean = x + step[:, None] * grad
    return x_mean + noise * torch.sqrt(step * 2)[:, None], x_mean


def langevin_step(p, sde, table, x, t, noise, snr, **fw):
    alpha = torch.ones_like(t) if sde.name == "VESDE" else (1.0 - table)[_timestep(sde, t)]
    grad = R.score_fn(p, sde, x, t, **fw)
    gn = torch.norm(grad.reshape(grad.shape[0], -1), dim=-1).mean()
    nn_ = torch.norm(noise.reshape(noise.shape[0], -1), dim=-1).mean()
    step = (snr * nn_ / gn) ** 2 * 2 * alpha
    x_mean = x + step[:, None] * grad
    return x_mean + torch.sqrt(step * 2)[:, None] * noise, x_mean


def noise_slots(corrector, n_steps_each, completion):
    """(number of slots per loop index, slot of the imputation after the corrector, of the predictor z, of the imputation after it)."""
    nc = 0 if corrector == "none" else n_steps_each
    return nc + (3 if completion else 1), nc, nc + (1 if completion else 0), nc + 2


def pc_loop(p, sde, x_init, draw, *, predictor, corrector, n_steps_each=1, snr=0.16, probability_flow=False, eps=1e-3, start_step=0,
            observation=None, mask=None, table=None, **fw):
    """Returns (trajs [n, B, D], x, x_mean, noise [n, slots, B, D] as the library takes it).  ``draw()`` returns the next [B, D] draw."""
    assert predictor in PREDICTORS and corrector in CORRECTORS
    x = x_init
    dt = x.dtype
    table = discrete_table(sde, dt) if table is None else torch.as_tensor(table).to(dt)
    timesteps = torch.linspace(sde.T, eps, sde.N).to(dt)                     # sampling.py:449
    completion = observation is not None
    k_slots, s_impa, s_pred, s_impb = noise_slots(corrector, n_steps_each, completion)
    n_run = sde.N - start_step
    noise = np.zeros((n_run, k_slots) + tuple(x.shape), np.float32)

    def take(i, slot):
        z = np.asarray(draw(), np.float32)
        noise[i - start_step, slot] = z
        return torch.tensor(z).to(dt)

    trajs = []
    x_mean = x
    for i in range(start_step, sde.N):
        vec_t = torch.ones(x.shape[0], dtype=dt) * timesteps[i]              # :458
        for k in range(0 if corrector == "none" else n_steps_each):
            step_fn = langevin_step if corrector == "langevin" else ald_step
            x, x_mean = step_fn(p, sde, table, x, vec_t, take(i, k), snr, **fw)
        if completion:
            x = R.impute(sde, x, vec_t, observation, mask, take(i, s_impa))
        if predictor == "euler_maruyama":
            z = take(i, s_pred)
            if probability_flow:
                drift, _, _ = R.rsde_sde(p, sde, x, vec_t, probability_flow=True, **fw)
                x_mean = x + drift * (-1.0 / sde.N)
                x = x_mean
            else:
                x, x_mean = R.em_step(p, sde, x, vec_t, z, **fw)
        elif predictor == "reverse_diffusion":
            x, x_mean = reverse_diffusion_step(p, sde, table, x, vec_t, take(i, s_pred), probability_flow, **fw)
        elif predictor == "ancestral_sampling":
            x, x_mean = ancestral_step(p, sde, table, x, vec_t, take(i, s_pred), **fw)
        else:
            x_mean = x                                                       # NonePredictor draws nothing
        if completion:
            x = R.impute(sde, x, vec_t, observation, mask, take(i, s_impb))
        trajs.append(x)
    return torch.stack(trajs, 0), x, x_mean, noise


# ---- (b) the stages on (float64 value, fp32 band) pairs ----------------------------------------------------------------------------------
def table_index(t32, N, T=1.0):
    """(t * (N - 1) / T).long(): two rounded fp32 operations and a truncation."""
    a = (np.asarray(t32, F32) * F32(N - 1)).astype(F32)
    return np.trunc((a / F32(T)).astype(F32).astype(np.float64)).astype(np.int64)


def table_entries(kind, t32, N, table32, T=1.0, adj_shift=0):
    """dict(tab, adj: E with zero bound -- the entries are fp32 numbers, exact; k: the index).  adj: VE's adjacent sigma, 0 at timestep 0.
    adj_shift seeds the off-by-one fault (adjacent index k - 1 + adj_shift)."""
    k = table_index(t32, N, T)
    tab = np.asarray(table32, np.float64)
    out = dict(k=k, tab=S.E(tab[k]), adj=S.E(np.zeros(np.shape(k))))
    if kind.startswith("ve"):
        ka = np.clip(k - 1 + adj_shift, 0, N - 1)
        out["adj"] = S.E(np.where(k == 0, 0.0, tab[ka]))
    return out


def base_kind(kind):
    return "ve" if kind.startswith("ve") else ("vp" if kind.startswith("vp") else "subvp")


def score_of(kind, s, usig, c):
    """The score behind a network whose output is c (model.py:194, utils.py:162 / :180)."""
    return S._score(kind, S.E(c) / usig, s["sd_score"])


def _impute(s, x, obs, mask, z):
    m = S.E(mask)
    return x * (1.0 - m) + (s["mc"] * S.E(obs) + S.E.of(z) * s["sd"]) * m


def _sqrt_1m(beta, linear_sqrt):
    return 1.0 - beta / 2.0 if linear_sqrt else S.sqrt(1.0 - beta)


def predictor_stage(predictor, kind, s, tb, score, x, z, N, pf=False, obs=None, mask=None, z_imp_b=None, pf_factor=1.0, linear_sqrt=False):
    """k_pc_pred_update: dict(x_mean, x) of one predictor step (and the imputation after it).  s: sde_ref.scalars (columns), tb:
    table_entries (columns)."""
    x = S.E.of(x)
    base = base_kind(kind)
    if predictor == "reverse_diffusion":
        if base == "vp":                                                     # DDPM: f = sqrt(alpha) x - x, G = sqrt(beta)
            f, G = _sqrt_1m(tb["tab"], linear_sqrt) * x - x, S.sqrt(tb["tab"])
        elif base == "ve":                                                   # SMLD: f = 0, G = sqrt(sigma^2 - adjacent^2)
            f, G = None, S.sqrt(tb["tab"] * tb["tab"] - tb["adj"] * tb["adj"])
        else:                                                                # drift dt, diffusion sqrt(dt)
            f, G = ((-0.5 * s["beta"]) * x) * S.const(1.0 / N), s["g"] * S.sqrt(S.const(1.0 / N))
        gs = (G * G) * score
        if pf_factor != 1.0:
            gs = gs * pf_factor
        rev_f = -gs if f is None else f - gs                                 # (0 - a is exact)
        x_mean = x - rev_f
        xn = x_mean if pf else x_mean + G * S.E.of(z)
    elif predictor == "ancestral_sampling":
        assert base != "subvp" and not pf
        if base == "ve":
            s2, a2 = tb["tab"] * tb["tab"], tb["adj"] * tb["adj"]
            d = s2 - a2
            x_mean = x + score * d
            k0 = a2.v == 0.0
            arg = (a2 * d) / s2
            with np.errstate(divide="ignore", invalid="ignore"):
                std = S.sqrt(S.E(np.where(k0, 1.0, arg.v), np.where(k0, 0.0, arg.e)))
            std = S.E(np.where(k0, 0.0, std.v), np.where(k0, 0.0, std.e))   # timestep 0: exactly 0, zero bound
        else:
            x_mean = (x + tb["tab"] * score) / _sqrt_1m(tb["tab"], linear_sqrt)
            std = S.sqrt(tb["tab"])
        xn = x_mean + std * S.E.of(z)
    else:
        x_mean = xn = x
    if obs is not None:
        xn = _impute(s, xn, obs, mask, z_imp_b)
    return dict(x_mean=x_mean, x=xn)


def ald_stage(kind, s, tb, score, x, noise, snr, obs=None, mask=None, z_imp=None, drop_alpha=False):
    """k_ald_update: step = (snr std)^2 * 2 * alpha with marginal_prob's std and alpha = 1 - beta (1 for VE); the imputation after the
    corrector on request."""
    a = S.const(snr) * s["sd"]
    step = (a * a) * 2.0
    if not drop_alpha:
        step = step * (S.E(np.ones(())) if base_kind(kind) == "ve" else 1.0 - tb["tab"])
    nscale = S.sqrt(step * 2.0)
    x_mean = S.E.of(x) + step * score
    xn = x_mean + S.E.of(noise) * nscale
    if obs is not None:
        xn = _impute(s, xn, obs, mask, z_imp)
    return dict(x_mean=x_mean, x=xn)


# ---- golden g32: tags and inputs ---------------------------------------------------------------------------------------------------------
LONG = {"rd": "reverse_diffusion", "anc": "ancestral_sampling", "em": "euler_maruyama", "none": "none", "lang": "langevin", "ald": "ald"}


def parse_tag(tag):
    """'<kind>_<pred>_<corr>[n][_pf][_completion|_denoise][_N1000]_(fn|loop)' -> dict."""
    parts = tag.split("_")
    corr = parts[2].rstrip("0123456789")
    return dict(kind=parts[0], predictor=LONG[parts[1]], corrector=LONG[corr], pf="pf" in parts[3:], completion="completion" in parts[3:])


def case_inputs(g, tag):
    N, B, n_each, pf, start, z0_seed, n_draws, keep = (int(v) for v in g[f"{tag}_meta"])
    z0 = (float(g[f"{tag}_z0_scale"]) * np.random.RandomState(z0_seed).standard_normal((B, 63))).astype(np.float32)
    return dict(N=N, B=B, n_each=n_each, pf=bool(pf), start=start, n_draws=n_draws, keep=keep, z0=z0, eps=float(g[f"{tag}_eps"]))


def golden_cases():
    from helpers import load
    return [str(t) for t in load("g32_pc_variants")["cases"]]
