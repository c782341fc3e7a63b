"""GPU tests of the probability-flow sampler (dposer_pf_sampler: pc_sampler with probability_flow = True, Euler-Maruyama predictor,
corrector 'none') and of the interpolation task built on it: parity with the reference's own deterministic sampler (golden g28), the
discrete score functions and the Fourier embedding against the PF oracle loop (tests/pf_ref.py), determinism, the two kernel forms
(fused epilogue / update kernel), the host routing and tasks/interpolation.py."""
import numpy as np
import pytest
import torch

from gpu_common import DEV, make_model, t2n
from helpers import load, rel_err
from oracle import score_ref as R
from pf_ref import pf_sampler

pytestmark = pytest.mark.gpu
torch.set_num_threads(8)
TOLS = {"fp32": 1e-4, "bf16x3": 1e-4, "bf16": 1e-2}          # after the 1000-step sampler


def _dev(a):
    return torch.tensor(np.asarray(a), dtype=torch.float32, device=DEV)


def _sde(kind, N, sigma_min=0.01, sigma_max=50.0):
    from dposer_amd.algorithms.advanced import sde_lib
    if kind in ("ve", "ve_disc"):
        return sde_lib.VESDE(sigma_min, sigma_max, N)
    return sde_lib.VPSDE(0.1, 20.0, N) if kind in ("vp", "vp_disc") else sde_lib.subVPSDE(0.1, 20.0, N)


def _pf_fn(cfg, sde, B, eps=1e-3, continuous=True):
    from dposer_amd.algorithms.advanced import sampling
    cfg.sampling.probability_flow = True
    cfg.sampling.predictor = "euler_maruyama"
    cfg.sampling.corrector = "none"
    cfg.training.continuous = continuous
    return sampling.get_sampling_fn(cfg, sde, (B, 63), lambda v: v, eps, device=DEV)


class _Args:
    def __init__(self, task):
        self.task = task


@pytest.mark.parametrize("prec", ["fp32", "bf16x3", "bf16"])
@pytest.mark.parametrize("kind", ["subvp", "vp", "ve"])
def test_pf_sampler_matches_reference_golden(kind, prec):
    g = load("g28_pf_sampler")
    cfg, m, p = make_model(int(g["seed"]), precision=prec)
    tag = f"{kind}8"
    fn = _pf_fn(cfg, _sde(kind, 8), 16, eps=float(g[f"{tag}_eps"]))
    noise = torch.randn(8, 1, 16, 63, device=DEV)               # the stochastic layout: the predictor slot is present and ignored
    trajs, x = fn(m, z=_dev(g[f"{tag}_z0"]), noise=noise)
    assert trajs.shape == (8, 16, 63)
    assert rel_err(t2n(trajs), g[f"{tag}_trajs"]) < TOLS[prec]
    assert rel_err(t2n(x), g[f"{tag}_final"]) < TOLS[prec]
    _, x2 = fn(m, z=_dev(g[f"{tag}_z0"]))
    assert torch.equal(x, x2)


def test_pf_sampler_completion_and_denoise_golden():
    g = load("g28_pf_sampler")
    cfg, m, p = make_model(int(g["seed"]), precision="fp32")
    fn = _pf_fn(cfg, _sde("subvp", 8), 16, eps=float(g["comp8_eps"]))
    noise = _dev(g["comp8_noise"]).reshape(8, 3, 16, 63)       # per step: impute A, predictor z (not read), impute B
    trajs, x = fn(m, observation=_dev(g["comp8_obs"]), mask=_dev(g["comp8_mask"]), z=_dev(g["comp8_z0"]), args=_Args("completion"), noise=noise)
    assert rel_err(t2n(trajs), g["comp8_trajs"]) < 1e-4
    assert rel_err(t2n(x), g["comp8_final"]) < 1e-4
    noise[:, 1] = 1e3                                           # the predictor slots are never read
    trajs2, _ = fn(m, observation=_dev(g["comp8_obs"]), mask=_dev(g["comp8_mask"]), z=_dev(g["comp8_z0"]), args=_Args("completion"), noise=noise)
    assert torch.equal(trajs, trajs2)
    trajs, x = fn(m, z=_dev(g["den8_z0"]), start_step=int(g["den8_start_step"]), args=_Args("denoise"))
    assert trajs.shape == (5, 16, 63)
    assert rel_err(t2n(trajs), g["den8_trajs"]) < 1e-4
    assert rel_err(t2n(x), g["den8_final"]) < 1e-4


@pytest.mark.parametrize("prec", ["fp32", "bf16x3", "bf16"])
def test_pf_sampler_1000_steps_golden(prec):
    """sub-VP, N = 1000, eps = 1e-5 (demo.py:443): the update-kernel form (trajectory kept) and the fused-epilogue form (none)."""
    g = load("g28_pf_sampler")
    cfg, m, p = make_model(int(g["seed"]), precision=prec)
    fn = _pf_fn(cfg, _sde("subvp", 1000), 8, eps=float(g["pf1000_eps"]))
    z0 = _dev(g["pf1000_z0"])
    trajs, x = fn(m, z=z0, traj_stride=100)
    assert trajs.shape == (10, 8, 63)
    assert rel_err(t2n(trajs), g["pf1000_trajs"]) < TOLS[prec]
    assert rel_err(t2n(x), g["pf1000_final"]) < TOLS[prec]
    _, xf = fn(m, z=z0, traj_stride=0)
    assert rel_err(t2n(xf), g["pf1000_final"]) < TOLS[prec]


@pytest.mark.parametrize("kind,embedding", [("vp_disc", "positional"), ("ve_disc", "positional"), ("ve", "fourier"), ("subvp", "fourier")])
def test_pf_sampler_discrete_and_fourier_vs_oracle(kind, embedding):
    cfg, m, p = make_model(31, precision="fp32", embedding=embedding)
    N, B = 8, 40
    continuous = not kind.endswith("_disc")
    fn = _pf_fn(cfg, _sde(kind, N), B, continuous=continuous)
    rs = np.random.RandomState(8)
    z0 = (rs.standard_normal((B, 63)) * (50.0 if kind.startswith("ve") else 1.0)).astype(np.float32)
    trajs, x = fn(m, z=_dev(z0))
    if kind.startswith("ve"):
        so = R.VE(N=N, discrete=not continuous)
    else:
        so = (R.VP if kind.startswith("vp") else R.SubVP)(N=N, discrete=not continuous)
    ref_trajs, ref_x = pf_sampler(p, so, torch.tensor(z0), embedding_type=embedding)
    tol = 2e-3 if embedding == "fourier" else 1e-4            # (Fourier: sin / cos of arguments up to ~1e3: test_forward_fourier_ve_...)
    assert rel_err(t2n(trajs), ref_trajs.numpy()) < tol
    assert rel_err(t2n(x), ref_x.numpy()) < tol
    _, xf = fn(m, z=_dev(z0), traj_stride=0)                   # fused-epilogue form
    assert rel_err(t2n(xf), ref_x.numpy()) < tol


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_pf_sampler_is_deterministic_and_x_equals_x_mean(prec):
    from dposer_amd.algorithms.advanced import sampling
    cfg, m, p = make_model(32, precision=prec)
    sde = _sde("subvp", 12)
    z0 = torch.randn(300, 63, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    ts = torch.linspace(sde.T, 1e-5, sde.N)
    runs = []
    for seed, stride in ((1, 0), (1, 0), (987654321, 0), (1, 3), (5, 3)):
        traj, x, xm = sampling.fused_em_sample(m, sde, z0.clone(), ts, seed=seed, traj_stride=stride, probability_flow=True)
        assert torch.equal(x, xm)                               # the diffusion is zeros(1): x = x_mean
        assert torch.isfinite(x).all()
        if stride:
            assert traj.shape == (4, 300, 63) and torch.equal(traj[-1], x)
        runs.append(x)
    for r in runs[1:]:
        assert torch.equal(r, runs[0])                          # two calls, any seed, either form: the same bits
    _, xs, _ = sampling.fused_em_sample(m, sde, z0.clone(), ts, seed=1, traj_stride=0)
    assert not torch.equal(xs, runs[0])                         # (the stochastic sampler on the same inputs differs)


def test_pf_trajectory_form_gives_the_bits_of_the_fused_form():
    """traj_stride runs post_dense + k_em_update (two launches per step), none runs EpiEmStep (one): same arithmetic, same bits --
    and each call takes the form it should (GEMM launches counted by the library's profiler)."""
    from dposer_amd import _C
    for prec in ("fp32", "bf16x3", "bf16"):
        cfg, m, p = make_model(33, precision=prec)
        N, B = 10, 500
        fn = _pf_fn(cfg, _sde("vp", N), B, eps=1e-5)
        z0 = torch.randn(B, 63, device=DEV, generator=torch.Generator(device=DEV).manual_seed(4))
        kinds = []
        for stride in (0, 1):
            _C.profile_enable(True)
            out = fn(m, z=z0, traj_stride=stride)
            torch.cuda.synchronize()
            stats = _C.profile_collect()
            _C.profile_enable(False)
            kinds.append({k: v[1] for k, v in stats.items()})
            if stride == 0:
                x0 = out[1]
            else:
                trajs, x1 = out
        em = lambda d, s: sum(c for k, c in d.items() if s in k)
        # (one fp32 row-major GEMM per call builds the time table)
        assert em(kinds[0], "post_em_step") == N and em(kinds[1], "post_em_step") == 0, kinds
        assert em(kinds[1], "rowmajor") - em(kinds[0], "rowmajor") == N, kinds
        assert torch.equal(x0, x1), (prec, rel_err(t2n(x0), t2n(x1)))
        assert torch.equal(trajs[-1], x1)


def test_pc_sampler_probability_flow_never_reaches_the_generic_predictor(monkeypatch):
    from dposer_amd.algorithms.advanced import sampling

    def boom(*a, **k):
        raise AssertionError("generic predictor reached")

    monkeypatch.setattr(sampling, "shared_predictor_update_fn", boom)
    g = load("g28_pf_sampler")
    cfg, m, p = make_model(int(g["seed"]), precision="bf16")
    for kind in ("subvp", "ve"):
        fn = _pf_fn(cfg, _sde(kind, 8), 16)
        trajs, x = fn(m, z=_dev(g[f"{kind}8_z0"]))
        assert torch.isfinite(x).all() and trajs.shape == (8, 16, 63)
    fn = _pf_fn(cfg, _sde("subvp", 8), 16)
    _, x = fn(m, observation=_dev(g["comp8_obs"]), mask=_dev(g["comp8_mask"]), z=_dev(g["comp8_z0"]), args=_Args("completion"))
    assert torch.isfinite(x).all()
    _, x = fn(m, z=_dev(g["den8_z0"]), start_step=3, args=_Args("denoise"), traj_stride=0)
    assert torch.isfinite(x).all()
    cfg.sampling.corrector = "langevin"                         # PF + corrector stays on the generic loop (demo.py:442)
    fn = sampling.get_sampling_fn(cfg, _sde("subvp", 8), (16, 63), lambda v: v, 1e-3, device=DEV)
    with pytest.raises(AssertionError, match="generic predictor"):
        fn(m, z=_dev(g["subvp8_z0"]))


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_interpolate_decodes_all_segments_in_one_call(prec, capsys):
    from dposer_amd.algorithms.advanced import sampling
    from dposer_amd.tasks import interpolation as I
    cfg, m, p = make_model(34, precision=prec)
    sde = _sde("subvp", 1000)
    rs = np.random.RandomState(9)
    anchors = _dev(rs.standard_normal((4, 63)) * 0.8)
    epsilon = _dev(rs.choice([-1.0, 1.0], size=(4, 63)))      # Hutchinson probe fixed: the encode is repeatable
    calls = []
    real = sampling.fused_em_sample
    monkey = lambda *a, **k: calls.append(a[2].shape[0]) or real(*a, **k)
    sampling.fused_em_sample = monkey
    try:
        z, recon, frames = I.interpolate(m, sde, anchors, frames=60, encode_kw=dict(epsilon=epsilon))
    finally:
        sampling.fused_em_sample = real
    assert calls == [4, 3 * 60]                                 # one call for the anchors, ONE for all 180 frames
    assert z.shape == (4, 63) and recon.shape == (4, 63) and frames.shape == (3, 60, 63)
    assert torch.isfinite(frames).all()
    tol = TOLS[prec]
    # the ends of each segment are the anchors' latents: their frames are the anchors' reconstructions
    assert rel_err(t2n(frames[:, 0]), t2n(recon[:-1])) < tol
    assert rel_err(t2n(frames[:, -1]), t2n(recon[1:])) < tol
    # the one-call decode against one decode per segment (the reference's loop, demo.py:465-471)
    lat = I.slerp_segments(z, 60)
    per = torch.stack([I.decode(m, sde, lat[s]) for s in range(3)])
    assert rel_err(t2n(frames), t2n(per)) < tol
    bits_seg = torch.equal(frames, per)
    bits_ends = torch.equal(frames[:, 0], recon[:-1]) and torch.equal(frames[:, -1], recon[1:])
    with capsys.disabled():
        print(f"\n[interpolate {prec}] one call vs per-segment decodes: bits equal {bits_seg}; segment ends vs reconstructions: bits equal {bits_ends}")
    # encode is the likelihood route (demo.py:432): z is likelihood_fn's latent
    from dposer_amd.algorithms.advanced import likelihood
    _, z_ref, _ = likelihood.get_likelihood_fn(sde, lambda v: v, rtol=1e-4, atol=1e-4, eps=1e-4)(m, anchors, epsilon=epsilon)
    assert torch.equal(z, z_ref)
