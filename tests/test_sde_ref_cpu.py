"""The float64 reference of the SDE scalars and output stages (tests/sde_ref.py) is tested here, on the CPU, before it judges any kernel:

  fixture    the reference's own fp32 scalars (golden g8, linspace(1, 1e-3, 1000)) lie inside the band at every grid point; labels bit for bit
  stages     the project's torch-fp32 step-by-step expressions (the formulas of prior._prior_loss_unfused, _prior_loss_multi_unfused,
             _red_diff_unfused, utils.ScoreFn and sde_lib's classes, a constant "network") lie inside the band on the whole grids
  mutations  eight seeded faults each push at least one element outside the band -- a band that cannot see them is too wide
  table      the discrete-VP std table: sde_lib.VPSDE reproduces the reference's (golden g27) bit for bit, and the table the kernels'
             launch code forms (sde_dev.h, a stand-alone host program) is within 2 fp32 ulp of it for N in {8, 1000, 2000}
"""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import sde_ref as S
from helpers import _log_measured, load

torch.set_num_threads(8)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS5 = S.KINDS
B, D = 5, 63


def _sde(kind, N=1000):
    from dposer_amd.algorithms.advanced import sde_lib
    if kind.startswith("ve"):
        return sde_lib.VESDE(sigma_min=0.01, sigma_max=50.0, N=N)
    return (sde_lib.subVPSDE if kind == "subvp" else sde_lib.VPSDE)(0.1, 20.0, N)


def _table(N=1000):
    return load("g27_vp_tables")[f"sqrt_1m_alphas_cumprod_{N}"]


def _sigmas():
    from oracle import score_ref as R
    return np.asarray(R.sigma_table(), dtype=np.float32).reshape(-1)


def _grid(N=1000):
    """Both grids, the index boundaries and the half-way labels, as fp32."""
    mult = N - 1
    ts = [torch.linspace(1.0, 1e-3, 1000).numpy(), torch.linspace(1.0, 1e-5, 1000).numpy(), S.boundary_times(999), S.boundary_times(mult),
          S.half_times(N), np.asarray([1.0, 1e-5, 1e-3], np.float32)]
    return np.unique(np.concatenate(ts).astype(np.float32))


def _data(seed=7):
    rs = np.random.RandomState(seed)
    n = B * D
    x0, z = rs.standard_normal(n).astype(np.float32), rs.standard_normal(n).astype(np.float32)
    c = (rs.choice([-1.0, 1.0], n) * np.exp(rs.uniform(np.log(1e-2), np.log(4.0), n))).astype(np.float32)
    return x0[None], z[None], c[None]


def _check(name, got, ref):
    r = S.worst(got, ref)
    _log_measured("band_ratio_" + name, r)
    assert r <= 1.0, (name, r, int(np.argmax(S.ratio_any(got, ref))))
    return r


# ---- fixture ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["subvp", "vp", "ve"])
def test_reference_fp32_scalars_lie_inside_the_band(kind):
    g = load("g8_scalars")
    t = g["t"]
    s = S.scalars(kind, t)
    _check(f"{kind}_std", g[f"{kind}_std"], s["sd"])
    _check(f"{kind}_sigma", g[f"{kind}_sigma"], s["sd"])
    _check(f"{kind}_mean", g[f"{kind}_mean"][:, 0], s["mc"])                      # x = ones
    _check(f"{kind}_diffusion", g[f"{kind}_diffusion"], s["g"])
    _check(f"{kind}_drift", g[f"{kind}_drift"][:, 0], -0.5 * s["beta"])
    if kind == "ve":
        assert g["ve_alpha"].reshape(-1).tolist() == [1.0]
    else:
        _check(f"{kind}_alpha", g[f"{kind}_alpha"][:, 0], s["mc"])
        assert s["label"].tobytes() == g["temb_labels"].tobytes()                 # bit for bit
    # the band sees a relative error far below the plain one: at t = 1e-3 the fp32 std is off by ~1e-4 relative and still inside
    assert float(np.max(s["sd"].e / np.abs(s["sd"].v))) > 1e-5 or kind == "ve"


def test_only_t_equal_T_has_an_ambiguous_ve_index():
    """Under the continuous VE kind the sigma index is trunc(sigma(t)), decided by a powf.  On the sweeps' time values sigma(t) sits within
    its band of an integer at t = T alone (sigma(1) = 50): there both indices are admissible, everywhere else the index is exact."""
    t32 = _grid()
    amb = S.ambiguous_index(S.scalars("ve", t32)["label"])
    assert t32[amb].tolist() == [1.0]


# ---- stages -------------------------------------------------------------------------------------------------------------------------
class _Net(torch.nn.Module):
    """The constant 'network' behind model.py:192-194: c / used_sigma(label)."""

    def __init__(self, c, sigmas, scale, fourier=False):
        super().__init__()
        self.c, self.sig, self.scale, self.fourier = torch.tensor(c), torch.tensor(sigmas), scale, fourier

    def forward(self, x, labels, condition=None, mask=None):
        if not self.scale:
            return self.c.expand(x.shape)
        used = labels.float() if self.fourier else self.sig[labels.long()]
        return self.c / used[:, None]


def _torch_stage(kind, t32, x0, z, c, scale, weighted, N=1000):
    """The formulas of _prior_loss_unfused / _prior_loss_multi_unfused (n = 2) / _red_diff_unfused, rows = time values, torch fp32."""
    from dposer_amd.algorithms.advanced import utils as mutils
    sde = _sde(kind, N)
    G = len(t32)
    t = torch.tensor(t32)
    X0, Z = torch.tensor(x0).expand(G, -1), torch.tensor(z).expand(G, -1)
    score_fn = mutils.get_score_fn(sde, _Net(c, _sigmas(), scale), train=False, continuous=kind in ("subvp", "vp", "ve"))
    inv_n = 1.0 / X0.shape[1]
    out = {}
    with torch.no_grad():
        mean, std = sde.marginal_prob(X0, t)
        x_t = mean + std[:, None] * Z
        score = score_fn(x_t, t, condition=None, mask=None)
        alpha, sigma = sde.return_alpha_sigma(t)
        x0_hat = (x_t + (sigma ** 2)[:, None] * score) / alpha
        snr = alpha / sigma[:, None]
        w = 0.5 * torch.sqrt(1 + snr) if weighted else torch.full_like(snr, 0.5)
        out["x_t"], out["x0_hat"] = x_t, x0_hat
        out["loss"] = (w * (X0 - x0_hat) ** 2).sum(1) * inv_n
        out["grad"] = 2 * w * (X0 - x0_hat) * inv_n
        # RED-Diff, motion_denoising.py:145-154
        resid = -score * std[:, None] - Z
        weight = torch.sqrt(sigma ** 2) / (alpha[:, 0] if alpha.shape[0] == G else alpha[0, 0])
        out["red_eps"] = -score * std[:, None]
        out["red_loss"] = weight * torch.einsum("ij,ij->i", resid, X0)
        out["red_grad"] = weight[:, None] * resid
        # two DDIM steps t -> 0.625 t -> 0.25 t (completion.py:112-129; the grid of linear_interpolation(t, t / 4, 3))
        traj = [t, (t + (t / 4 - t) * 0.5), t / 4]
        x = x_t
        for i in range(2):
            a_c, s_c = sde.return_alpha_sigma(traj[i])
            a_b, s_b = sde.return_alpha_sigma(traj[i + 1])
            noise = -score_fn(x, traj[i], condition=None, mask=None) * s_c[:, None]
            x = a_b / a_c * (x - s_c[:, None] * noise) + s_b[:, None] * noise
        out["ddim_x0_hat"] = x
        out["ddim_loss"] = (w * (X0 - x) ** 2).sum(1) * inv_n
    return {k: v.numpy() for k, v in out.items()}


def _ref_stage(kind, t32, x0, z, c, scale, weighted, N=1000, side=0):
    sig = _sigmas()
    tab = _table(N) if kind == "vp_discrete" else None
    sc = lambda tt: S._col(S.scalars(kind, tt, N=N, table=tab))
    us = lambda s: S.used_sigma(sig, s["label"][..., None] if not isinstance(s["label"], S.E) else s["label"], False, scale, side)
    s = sc(t32)
    inv_n = 1.0 / x0.shape[1]
    d = S.denoise(kind, s, us(s), x0, z, c, weighted, inv_n, per_row=True)
    r = S.red_diff(kind, s, us(s), x0, z, c, per_row=True, inv_batch=1.0)
    t = torch.tensor(t32)
    traj = [t.numpy(), (t + (t / 4 - t) * 0.5).numpy(), (t / 4).numpy()]
    ss = [sc(tt) for tt in traj]
    m = S.ddim(kind, ss, [us(v) for v in ss], x0, z, c, weighted, inv_n, per_row=True)
    return dict(x_t=d["x_t"], x0_hat=d["x0_hat"], loss=d["loss"], grad=d["grad"], red_eps=r["eps_pred"], red_loss=r["loss"],
                red_grad=r["grad"], ddim_x0_hat=m["x0_hat"], ddim_loss=m["loss"])


@pytest.mark.parametrize("kind,N,scale", [(k, 1000, sc) for k in KINDS5 for sc in (True, False)] + [("vp_discrete", 2000, False)])
def test_torch_fp32_stages_lie_inside_the_band(kind, N, scale):
    """'The reference alone stays within the band': one-step denoise (weighted and not), RED-Diff and a two-step DDIM estimate in torch
    fp32 on both grids, the index boundaries and the half-way labels.  (N = 2000: labels pass the 1000 sigmas; without scale_by_sigma only,
    as the reference's lookup would raise.)"""
    x0, z, c = _data()
    t32 = _grid(N)
    for weighted in (True, False):
        got = _torch_stage(kind, t32, x0, z, c, scale, weighted, N)
        refs = [_ref_stage(kind, t32, x0, z, c, scale, weighted, N, side) for side in ((-1, 1) if kind == "ve" else (0,))]
        for k in refs[0]:
            _check(f"{kind}_{N}_{k}", got[k], [r[k] for r in refs])


@pytest.mark.parametrize("kind,N,scale", [(k, 1000, sc) for k in KINDS5 for sc in (True, False)] + [("vp_discrete", 2000, False)])
def test_torch_fp32_em_step_lies_inside_the_band(kind, N, scale):
    """One Euler-Maruyama predictor step (sampling.py:182-188 over sde_lib's reverse SDE), plain and under probability flow, torch fp32."""
    from dposer_amd.algorithms.advanced import utils as mutils
    x, z, c = _data(9)
    t32 = _grid(N)
    G, t = len(t32), torch.tensor(_grid(N))
    sde = _sde(kind, N)
    score_fn = mutils.get_score_fn(sde, _Net(c, _sigmas(), scale), train=False, continuous=kind in ("subvp", "vp", "ve"))
    X, Z = torch.tensor(x).expand(G, -1), torch.tensor(z).expand(G, -1)
    for pf in (False, True):
        rsde = sde.reverse(score_fn, probability_flow=pf)
        with torch.no_grad():
            dt = -1.0 / rsde.N
            drift, diffusion = rsde.sde(X, t)
            x_mean = X + drift * dt
            xn = x_mean + diffusion[:, None] * np.sqrt(-dt) * Z
        refs = []
        for side in ((-1, 1) if kind == "ve" else (0,)):
            s = S._col(S.scalars(kind, t32, N=N, table=_table(N) if kind == "vp_discrete" else None))
            lab = s["label"] if isinstance(s["label"], S.E) else s["label"][:, None]
            refs.append(S.em_update(kind, s, None, S.used_sigma(_sigmas(), lab, False, scale, side), x, c, z, N=N, pf=pf))
        _check(f"em_{kind}_{N}_pf{int(pf)}_x_mean", x_mean.numpy(), [r["x_mean"] for r in refs])
        _check(f"em_{kind}_{N}_pf{int(pf)}_x", xn.numpy(), [r["x"] for r in refs])


@pytest.mark.parametrize("kind", ["subvp", "vp", "ve"])
def test_torch_fp32_pf_rhs_lies_inside_the_band(kind):
    """likelihood.py:60-65, 86-95 in torch fp32: the drift of the probability-flow ODE, autograd's gradient of sum(drift * noise) w.r.t. the
    network output, and the Hutchinson sum formed from a given input gradient."""
    x, nz, out = _data(13)
    dx = _data(14)[0]
    t32 = _grid()
    G, t = len(t32), torch.tensor(t32)
    sde = _sde(kind)
    leaf = torch.tensor(out).expand(G, -1).clone().requires_grad_(True)

    class Net(torch.nn.Module):
        def forward(self, xx, labels, condition=None, mask=None):
            return leaf

    from dposer_amd.algorithms.advanced import utils as mutils
    rsde = sde.reverse(mutils.get_score_fn(sde, Net(), train=False, continuous=True), probability_flow=True)
    X, NZ = torch.tensor(x).expand(G, -1), torch.tensor(nz).expand(G, -1)
    drift = rsde.sde(X, t)[0]
    (drift * NZ).sum().backward()
    a = torch.zeros(G, 1) if kind == "ve" else -0.5 * sde._beta(t)[:, None]
    hutch = ((torch.tensor(dx) + NZ * a) * NZ).sum(1)
    ref = S.pf_rhs(kind, S._col(S.scalars(kind, t32)), x, out, nz, dx)
    _check(f"pf_{kind}_drift", drift.detach().numpy(), ref["drift"])
    _check(f"pf_{kind}_dout", leaf.grad.numpy(), ref["dout"])
    _check(f"pf_{kind}_hutch", hutch.numpy(), ref["hutch"])


@pytest.mark.parametrize("scale", [True, False])
@pytest.mark.parametrize("kind", ["subvp", "vp", "ve"])
def test_torch_fp32_dsm_step_lies_inside_the_band(kind, scale):
    """losses.py:110-131 in torch fp32 with every grid value as the t of one row: the loss, autograd's gradient w.r.t. the network output
    (dres) and its column sums (added in float64 from the fp32 dres: torch's own order of a column sum is not the kernel's)."""
    _, z1, c = _data(15)
    t32 = _grid()
    G = len(t32)
    z = np.random.RandomState(16).standard_normal((G, z1.shape[1])).astype(np.float32)
    sde = _sde(kind)
    t = torch.tensor(t32)
    leaf = torch.tensor(c).expand(G, -1).clone().requires_grad_(True)
    labels = sde.marginal_prob(torch.zeros(G, 1), t)[1] if kind == "ve" else t * 999
    used = torch.tensor(_sigmas())[labels.long()][:, None] if scale else torch.ones(G, 1)
    std = sde.marginal_prob(torch.zeros(G, 1), t)[1][:, None]
    model = leaf / used
    score = model if kind == "ve" else -model / std
    loss = torch.mean(torch.square(score * std + torch.tensor(z)))
    loss.backward()
    refs = []
    for side in ((-1, 1) if (kind == "ve" and scale) else (0,)):
        s = S._col(S.scalars(kind, t32))
        lab = s["label"] if isinstance(s["label"], S.E) else s["label"][:, None]
        refs.append(S.dsm(kind, s, S.used_sigma(_sigmas(), lab, False, scale, side), c, z))
    tag = f"dsm_{kind}_{'scaled' if scale else 'raw'}"
    _check(f"{tag}_loss", loss.detach().numpy(), [r["loss"] for r in refs])
    _check(f"{tag}_dres", leaf.grad.numpy(), [r["dres"] for r in refs])
    _check(f"{tag}_bias_grad", leaf.grad.numpy().astype(np.float64).sum(0), [r["bias_grad"] for r in refs])


@pytest.mark.parametrize("kind,N", [(k, 1000) for k in KINDS5])
def test_torch_fp32_langevin_step_lies_inside_the_band(kind, N):
    """LangevinCorrector.update_fn (sampling.py:282-302) in torch fp32 over the score function, rows = time values."""
    from dposer_amd.algorithms.advanced import utils as mutils
    rs = np.random.RandomState(21)
    x, nz = (rs.standard_normal((B, D)).astype(np.float32) for _ in range(2))
    c = np.broadcast_to(_data(22)[2][0, :D], (B, D)).copy()
    t32 = _grid(N)
    G = len(t32)
    sde = _sde(kind, N)
    snr, alpha = 0.16, 0.97

    class Net(torch.nn.Module):
        def forward(self, xx, labels, condition=None, mask=None):
            return torch.tensor(c).reshape(1, -1).expand(xx.shape[0], -1)

    score_fn = mutils.get_score_fn(sde, Net(), train=False, continuous=kind in ("subvp", "vp", "ve"))
    with torch.no_grad():
        X = torch.tensor(x).reshape(1, -1).expand(G, -1)
        grad = score_fn(X, torch.tensor(t32)).reshape(G, B, D)
        noise = torch.tensor(nz).expand(G, B, D)
        grad_norm = torch.norm(grad.reshape(G, B, -1), dim=-1).mean(-1)
        noise_norm = torch.norm(noise.reshape(G, B, -1), dim=-1).mean(-1)
        step = (snr * noise_norm / grad_norm) ** 2 * 2 * alpha
        x_mean = torch.tensor(x) + step[:, None, None] * grad
        xn = x_mean + torch.sqrt(step * 2)[:, None, None] * noise
    s = S._col(S.scalars(kind, t32, N=N, table=_table(N) if kind == "vp_discrete" else None), 2)
    ref = S.langevin(kind, s, S.E(np.ones((G, 1, 1))), x[None], c[None], np.broadcast_to(nz, (G, B, D)), snr, alpha)
    _check(f"langevin_{kind}_gsum", (grad_norm * B).numpy(), ref["gsum"])
    _check(f"langevin_{kind}_x_mean", x_mean.numpy(), ref["x_mean"])
    _check(f"langevin_{kind}_x", xn.numpy(), ref["x"])


@pytest.mark.parametrize("kind", KINDS5)
def test_torch_fp32_completion_adam_step_lies_inside_the_band(kind):
    """One step of DPoserComp.optimize (completion.py:131-149, 195-201) in torch fp32: the loss formulas of _prior_loss_unfused, autograd's
    gradient and torch.optim.Adam started from given (non-zero) moments, rows = time values -- from zero moments Adam's first step is
    lr sign(g) whatever the scalars are."""
    from dposer_amd.algorithms.advanced import utils as mutils
    x0, z, c = _data(31)
    rs = np.random.RandomState(32)
    n = B * D
    obs = rs.standard_normal((1, n)).astype(np.float32)
    mask = (rs.uniform(size=(1, n)) < 0.5).astype(np.float32)
    m0 = (1e-3 * rs.standard_normal((1, n))).astype(np.float32)
    v0 = (1e-6 * rs.uniform(0.5, 2.0, (1, n))).astype(np.float32)
    t32 = _grid()[::3]
    G, t = len(t32), torch.tensor(_grid()[::3])
    sde = _sde(kind)
    score_fn = mutils.get_score_fn(sde, _Net(c, _sigmas(), True), train=False, continuous=kind in ("subvp", "vp", "ve"))
    lr, w_prior, w_data = 0.1, 0.7, 1.3
    for weighted in (True, False):
        x = torch.tensor(x0).expand(G, -1).clone().requires_grad_(True)
        Z, OBS, MK = torch.tensor(z).expand(G, -1), torch.tensor(obs).expand(G, -1), torch.tensor(mask).expand(G, -1)
        with torch.no_grad():
            mean, std = sde.marginal_prob(x.detach(), t)
            x_t = mean + std[:, None] * Z
            score = score_fn(x_t, t, condition=None, mask=None)
            alpha, sigma = sde.return_alpha_sigma(t)
            x0_hat = (x_t + (sigma ** 2)[:, None] * score) / alpha
            snr = alpha / sigma[:, None]
            w = 0.5 * torch.sqrt(1 + snr) if weighted else torch.full_like(snr, 0.5)
        loss = w_prior * (w * (x - x0_hat) ** 2).mean(1).sum() + w_data * ((x * MK - OBS * MK) ** 2).mean(1).sum()
        opt = torch.optim.Adam([x], lr, betas=(0.9, 0.999))
        opt.state[x] = dict(step=torch.tensor(0.0), exp_avg=torch.tensor(m0).expand(G, -1).clone(),
                            exp_avg_sq=torch.tensor(v0).expand(G, -1).clone())
        loss.backward()
        opt.step()
        s = S._col(S.scalars(kind, t32, table=_table() if kind == "vp_discrete" else None))
        refs = []
        for side in ((-1, 1) if kind == "ve" else (0,)):
            lab = s["label"] if isinstance(s["label"], S.E) else s["label"][:, None]
            refs.append(S.completion_update(kind, s, S.used_sigma(_sigmas(), lab, False, True, side), x0.reshape(1, 1, n), z.reshape(1, 1, n),
                                            c.reshape(1, 1, n), obs.reshape(1, 1, n), mask.reshape(1, 1, n), m0.reshape(1, 1, n),
                                            v0.reshape(1, 1, n), weighted, w_prior, w_data, lr, 0.9, 0.999, 1e-8))
        # (the reference's [..., B, D] layout with B = 1 row of n: scalars as [G, 1, 1])
        fix = lambda e: S.E(e.v.reshape(G, n), e.e.reshape(G, n))
        _check(f"completion_{kind}_x", x.detach().numpy(), [fix(r["x"]) for r in refs])
        _check(f"completion_{kind}_m", opt.state[x]["exp_avg"].numpy(), [fix(r["m"]) for r in refs])
        _check(f"completion_{kind}_v", opt.state[x]["exp_avg_sq"].numpy(), [fix(r["v"]) for r in refs])


# ---- mutations ----------------------------------------------------------------------------------------------------------------------
def _outside(got, ref):
    return S.worst(got.v if isinstance(got, S.E) else got, ref) > 1.0


def test_mutation_label_index_off_by_one_at_a_boundary():
    sig = _sigmas()
    c = _data()[2]
    for mult, kind, N in ((999, "subvp", 1000), (999, "vp_discrete", 1000)):
        t32 = S.boundary_times(mult)
        good = S.scalars(kind, t32, N=N, table=_table(N))
        bad = S.scalars(kind, t32, N=N, table=_table(N), label_shift=1)
        ref = S.out_model(c, S.used_sigma(sig, good["label"][:, None], False))
        assert _outside(S.out_model(c, S.used_sigma(sig, bad["label"][:, None], False)), ref)
        # and the two sides of every boundary are told apart: adjacent fp32 t, different sigma
        idx = S.sigma_index(good["label"], len(sig))
        assert len(np.unique(idx)) >= 9


def test_mutation_fp32_running_product_table():
    g = load("g27_vp_tables")
    N = 1000
    alphas = (np.float32(1.0) - g[f"discrete_betas_{N}"]).astype(np.float32)
    prod, run = np.empty(N, np.float32), np.float32(1.0)
    for i in range(N):
        run = np.float32(run * alphas[i])
        prod[i] = run
    bad_table = np.sqrt((np.float32(1.0) - prod).astype(np.float32)).astype(np.float32)
    x0, z, c = _data()
    t32 = torch.linspace(1.0, 1e-3, 1000).numpy()
    sig = _sigmas()
    outs = []
    for tab in (_table(N), bad_table):
        # One Euler-Maruyama step without scale_by_sigma.  Where the score meets marginal_prob's own std (x0_hat: sigma^2 score, RED-Diff:
        # score std) the fp32 cancellation of 1 - exp(2 lmc) at small t -- 1.5e-4 relative, inside the band by construction -- hides a
        # 4.3e-5 fault; the drift g^2 score dt has no such partner.  With scale_by_sigma the sigmas ~ 48 of the small indices shrink the
        # score's share of x_mean below x's own rounding.
        s = S._col(S.scalars("vp_discrete", t32, N=N, table=tab))
        outs.append(S.em_update("vp_discrete", s, None, S.used_sigma(sig, s["label"][..., None], False, False), x0, c, z, N=N))
    r = S.ratio(outs[1]["x_mean"].v, outs[0]["x_mean"]).max(axis=1)
    _log_measured("mutation_fp32_table_ratio", float(r.max()))
    assert r.max() > 1.0
    assert int(S.label_vp(t32, N - 1)[np.argmax(r)]) < 16                           # the fault sits at the small indices (4.3e-5 at index 4)


def _shared(kind, t, N=1000):
    s = S.scalars(kind, np.float32(t), N=N, table=_table(N) if kind == "vp_discrete" else None)
    lab = s["label"]
    return s, S.used_sigma(_sigmas(), lab, False)


def test_mutation_probability_flow_factor():
    x0, z, c = (a.reshape(B, D) for a in _data())
    for kind in ("subvp", "vp", "ve"):
        s, us = _shared(kind, 0.5)
        ref = S.em_update(kind, s, None, us, x0, c, z, pf=True)
        assert _outside(S.em_update(kind, s, None, us, x0, c, z, pf=True, pf_factor=1.0)["x"], ref["x"])


def test_mutation_weighted_ignored():
    x0, z, c = (a.reshape(B, D) for a in _data())
    for kind in KINDS5:
        s, us = _shared(kind, 0.3)
        ref = S.denoise(kind, s, us, x0, z, c, False, 1.0 / (B * D))
        bad = S.denoise(kind, s, us, x0, z, c, False, 1.0 / (B * D), ignore_weighted=True)
        assert _outside(bad["loss"], ref["loss"]) and _outside(bad["grad"], ref["grad"])


def test_mutation_sd_score_swapped_for_sd_under_vp_discrete():
    x0, z, c = (a.reshape(B, D) for a in _data())
    hit = 0
    for t in torch.linspace(1.0, 1e-3, 1000).numpy()[::37]:
        good = S.scalars("vp_discrete", np.float32(t), table=_table())
        bad = S.scalars("vp_discrete", np.float32(t), table=_table(), sd_score_is_sd=True)
        us = S.used_sigma(_sigmas(), good["label"], False)
        ref = S.denoise("vp_discrete", good, us, x0, z, c, True, 1.0 / (B * D))
        hit += _outside(S.denoise("vp_discrete", bad, us, x0, z, c, True, 1.0 / (B * D))["x0_hat"], ref["x0_hat"])
    assert hit >= 20          # the table's std is the marginal std of the step BELOW t: apart at (nearly) every t, not at a lucky one


def test_mutation_t_next_imputation_scalars_taken_at_t():
    x0, z, c = (a.reshape(B, D) for a in _data())
    rs = np.random.RandomState(3)
    obs, zb, za = (rs.standard_normal((B, D)).astype(np.float32) for _ in range(3))
    mask = (rs.uniform(size=(B, D)) < 0.5).astype(np.float32)
    grid = torch.linspace(1.0, 1e-3, 1000).numpy()
    for kind in ("subvp", "vp", "ve"):
        for i in (0, 500, 998):
            s, us = _shared(kind, grid[i])
            s_next, _ = _shared(kind, grid[i + 1])
            ref = S.em_update(kind, s, s_next, us, x0, c, z, obs=obs, mask=mask, z_imp_b=zb, z_imp_a=za)
            bad = S.em_update(kind, s, s, us, x0, c, z, obs=obs, mask=mask, z_imp_b=zb, z_imp_a=za)
            assert _outside(bad["x"], ref["x"]), (kind, i)


def test_mutation_ddim_last_step_weight_taken_at_t():
    x0, z, c = (a.reshape(B, D) for a in _data())
    from dposer_amd.prior import multi_step_time_grid
    for kind in ("subvp", "vp", "ve"):
        traj = np.asarray(multi_step_time_grid(0.4, 5), np.float32)
        ss = [S.scalars(kind, tt) for tt in traj]
        us = [S.used_sigma(_sigmas(), s["label"], False) for s in ss]
        ref = S.ddim(kind, ss, us, x0, z, c, True, 1.0 / (B * D))
        bad = S.ddim(kind, ss, us, x0, z, c, True, 1.0 / (B * D), weight_at_last=True)
        assert _outside(bad["loss"], ref["loss"]) and _outside(bad["grad"], ref["grad"])
        assert not _outside(bad["x0_hat"], ref["x0_hat"])


def test_mutation_round_half_up_in_the_ve_discrete_label():
    t32 = S.half_times(1000)
    assert len(t32) == 8
    good, bad = S.label_ve_discrete(t32), S.label_ve_discrete(t32, half_up=True)
    assert (good % 2 == 0).all() and (good != bad).sum() == 4                       # the four even k: half-even stays, half-up moves
    c = _data()[2]
    sig = _sigmas()
    ref = S.out_model(c, S.used_sigma(sig, good[:, None], False))
    assert _outside(S.out_model(c, S.used_sigma(sig, bad[:, None], False)), ref)


# ---- the discrete-VP table ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [8, 1000, 2000])
def test_vpsde_reproduces_the_reference_tables_bit_for_bit(N):
    g = load("g27_vp_tables")
    sde = _sde("vp", N)
    assert sde.discrete_betas.numpy().tobytes() == g[f"discrete_betas_{N}"].tobytes()
    assert sde.sqrt_1m_alphas_cumprod.numpy().tobytes() == g[f"sqrt_1m_alphas_cumprod_{N}"].tobytes()


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_kernel_side_table_is_within_2_ulp_of_the_reference(tmp_path):
    """tests/sde_table_main.hip includes sde_dev.h and prints what the launch code hands to the kernels (directly, and through
    make_sde_dev_at at a t of every index).  Bound: 2 fp32 ulp of the fixture.  The product is accumulated in double like torch.cumprod's
    on the CPU; the betas are linspace's two-ended fp32 formula, up to 1 ulp from torch's vectorised one, which moves 1 - beta in fp32 at
    two entries per table.  Measured: 0 / 1 / 1 ulp (N = 8 / 1000 / 2000); the fp32 running product before: 0 / 605 / 924 ulp at index 4."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "sde_table")
    cc = subprocess.run([hipcc, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "dposer_amd", "csrc"),
                         os.path.join(ROOT, "tests", "sde_table_main.hip"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stdout + cc.stderr
    rows = subprocess.run([exe, "8", "1000", "2000"], check=True, capture_output=True, text=True, timeout=60).stdout.split("\n")
    rows = np.asarray([[int(r.split()[0]), int(r.split()[1]), int(r.split()[2], 16), int(r.split()[3], 16)] for r in rows if r], np.int64)
    g = load("g27_vp_tables")
    for N in (8, 1000, 2000):
        sel = rows[rows[:, 0] == N]
        assert sel[:, 1].tolist() == list(range(N))
        direct, at = sel[:, 2].astype(np.uint32).view(np.float32), sel[:, 3].astype(np.uint32).view(np.float32)
        assert direct.tobytes() == at.tobytes()
        tab = g[f"sqrt_1m_alphas_cumprod_{N}"]
        ulps = np.abs(direct.astype(np.float64) - tab) / np.spacing(tab)
        _log_measured(f"vp_table_ulp_{N}", float(ulps.max()))
        assert ulps.max() <= 2.0, (N, float(ulps.max()), int(ulps.argmax()))
