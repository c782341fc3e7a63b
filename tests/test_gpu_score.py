"""GPU parity tests of the score path: HIP kernels (through the C ABI) vs the CPU oracle and vs the
golden vectors captured from the reference.  Tolerances: gpu_common.TOL_FP32 / TOL_BF16."""
import os
import numpy as np
import pytest
import torch

from gpu_common import DEV, TOL_BF16, TOL_FP32, make_model, t2n
from helpers import load, masks_from_keep, probe, rel_err
from oracle import philox as PH
from oracle import score_ref as R

pytestmark = pytest.mark.gpu
torch.set_num_threads(8)


def _dev(a):
    return torch.tensor(np.asarray(a), dtype=torch.float32, device=DEV)


# ------------------------------------------------------------------------------------------------
# ScoreModelFC.forward / get_score_fn vs reference goldens
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec,tol", [("fp32", TOL_FP32), ("bf16", TOL_BF16), ("bf16x3", TOL_FP32)])
@pytest.mark.parametrize("tag,D", [("axis_pos", 63), ("rot6d_pos", 126)])
def test_forward_matches_reference_golden(tag, D, prec, tol):
    from dposer_amd.algorithms.advanced import sde_lib
    from dposer_amd.algorithms.advanced import utils as mutils
    g = load("g1_forward")
    cfg, m, p = make_model(int(g[f"{tag}_seed"]), D=D, precision=prec)
    x, t = _dev(g[f"{tag}_x"]), _dev(g[f"{tag}_t"])
    with torch.no_grad():
        out = m(x, t * 999)
        assert rel_err(t2n(out), g[f"{tag}_model"]) < tol
        for name, sde in (("subvp", sde_lib.subVPSDE(0.1, 20.0, 1000)), ("vp", sde_lib.VPSDE(0.1, 20.0, 1000))):
            fn = mutils.get_score_fn(sde, m, train=False, continuous=True)
            assert rel_err(t2n(fn(x, t, None, None)), g[f"{tag}_score_{name}"]) < tol


def test_forward_fourier_ve_matches_reference_golden():
    from dposer_amd.algorithms.advanced import sde_lib
    from dposer_amd.algorithms.advanced import utils as mutils
    g = load("g1_forward")
    cfg, m, p = make_model(int(g["axis_fourier_seed"]), precision="fp32", embedding="fourier")
    x, t = _dev(g["axis_fourier_x"]), _dev(g["axis_fourier_t"])
    fn = mutils.get_score_fn(sde_lib.VESDE(0.01, 50.0, 1000), m, train=False, continuous=True)
    with torch.no_grad():
        out = fn(x, t, None, None)
    # sin/cos of arguments up to ~1e3 * 2 pi: one fp32 ulp of the argument is 6e-5 absolute
    assert rel_err(t2n(out), g["axis_fourier_score_ve"]) < 2e-3


def test_empty_batches():
    """B = 0: torch's layers and loops (the reference) return empty tensors; the kernels take B >= 1, so the host mirror answers itself:
    forward and sampler return empties of the right shape, the training step and the prior loss (NaN in the reference: a mean over
    nothing) refuse."""
    from dposer_amd.algorithms.advanced import sde_lib
    from dposer_amd.prior import prior_loss
    cfg, m, p = make_model(3, precision="bf16")
    x0 = torch.zeros(0, 63, device=DEV)
    assert m(x0, torch.zeros(0, device=DEV)).shape == (0, 63)
    m.train()
    xg = x0.clone().requires_grad_(True)
    out = m(xg, torch.zeros(0, device=DEV))
    assert out.shape == (0, 63)
    out.sum().backward()
    assert xg.grad.shape == (0, 63)
    m.eval()
    sde, fn = _sampler(m, cfg, 8, 0)
    trajs, x = fn(m, z=x0)
    assert x.shape == (0, 63) and trajs.shape[1:] == (0, 63)
    with pytest.raises(ValueError):
        _fused_grad(m, x0, None, None)
    with pytest.raises(ValueError):
        prior_loss(m, sde_lib.subVPSDE(0.1, 20.0, 1000), x0, 0.5)


@pytest.mark.parametrize("B", [1, 31, 33, 64, 100, 500, 513, 1000, 4096])
def test_forward_ragged_batches_vs_oracle(B):
    cfg, m, p = make_model(11, precision="fp32")
    rs = np.random.RandomState(B)
    x = rs.standard_normal((B, 63)).astype(np.float32)
    t = rs.uniform(1e-5, 1, B).astype(np.float32)
    with torch.no_grad():
        out = m(_dev(x), _dev(t) * 999)
    ref = R.scorefc_forward(p, torch.tensor(x), torch.tensor(t) * 999)
    assert rel_err(t2n(out), ref.numpy()) < TOL_FP32


def test_forward_is_batch_independent_at_full_size():
    """Size-independent property at the BASELINE batch (65536): a row's output does not depend on which
    tile / batch it is evaluated in (BIG 256x256 tiling vs SMALL tiling of a 48-row slice)."""
    cfg, m, p = make_model(12, precision="bf16")
    gen = torch.Generator(device=DEV).manual_seed(1)
    x = torch.randn(65536, 63, device=DEV, generator=gen)
    t = torch.rand(65536, device=DEV, generator=gen) * 0.999 + 1e-3
    with torch.no_grad():
        big = m(x, t * 999)
        sl = slice(40000, 40048)
        small = m(x[sl].contiguous(), (t[sl] * 999).contiguous())
    assert torch.isfinite(big).all()
    assert torch.equal(big[sl], small)


# ------------------------------------------------------------------------------------------------
# sampler
# ------------------------------------------------------------------------------------------------
def _sampler(m, cfg, N, B, corrector="none"):
    from dposer_amd.algorithms.advanced import sampling, sde_lib
    sde = sde_lib.subVPSDE(0.1, 20.0, N)
    cfg.sampling.corrector = corrector
    return sde, sampling.get_sampling_fn(cfg, sde, (B, 63), lambda x: x, 1e-3, device=DEV)


class _Args:
    def __init__(self, task):
        self.task = task


@pytest.mark.parametrize("prec,tol", [("fp32", 1e-4), ("bf16", 1e-2), ("bf16x3", 1e-4)])      # bf16 measured 4.0e-3
def test_em_sampler_matches_reference_golden(prec, tol):
    g = load("g5_sampler")
    cfg, m, p = make_model(int(g["seed"]), precision=prec)
    sde, fn = _sampler(m, cfg, 8, 16)
    noise = _dev(g["em8_noise"])[:, None]                       # [8, 1, B, D]
    trajs, x = fn(m, z=_dev(g["em8_z0"]), noise=noise)
    assert trajs.shape == (8, 16, 63)
    assert rel_err(t2n(trajs), g["em8_trajs"]) < tol
    assert rel_err(t2n(x), g["em8_final"]) < tol


def test_em_sampler_denoise_start_step_golden():
    g = load("g5_sampler")
    cfg, m, p = make_model(int(g["seed"]), precision="fp32")
    sde, fn = _sampler(m, cfg, 8, 16)
    trajs, x = fn(m, z=_dev(g["den8_z0"]), start_step=3, args=_Args("denoise"), noise=_dev(g["den8_noise"])[:, None])
    assert trajs.shape == (5, 16, 63)
    assert rel_err(t2n(trajs), g["den8_trajs"]) < 1e-4
    assert rel_err(t2n(x), g["den8_final"]) < 1e-4


def test_em_sampler_completion_golden():
    g = load("g5_sampler")
    cfg, m, p = make_model(int(g["seed"]), precision="fp32")
    sde, fn = _sampler(m, cfg, 8, 16)
    noise = _dev(g["comp8_noise"]).reshape(8, 3, 16, 63)        # per step: impute A, predictor z, impute B
    trajs, x = fn(m, observation=_dev(g["comp8_obs"]), mask=_dev(g["comp8_mask"]), z=_dev(g["comp8_z0"]), args=_Args("completion"),
                  noise=noise)
    assert rel_err(t2n(trajs), g["comp8_trajs"]) < 1e-4
    assert rel_err(t2n(x), g["comp8_final"]) < 1e-4
    mask = g["comp8_mask"]
    # imputed entries of the last state are a draw around the observation, the rest is the sampler's
    assert np.abs(t2n(trajs)[-1] * mask - g["comp8_trajs"][-1] * mask).max() < 1e-3


@pytest.mark.parametrize("prec,tol", [("fp32", 1e-5), ("bf16", 2e-2), ("bf16x3", 2e-5)])      # measured: fp32 2.0e-6, bf16 7.6e-3 (a gradient through the network)
def test_guided_em_step_matches_reference_golden(prec, tol, monkeypatch):
    """EulerMaruyamaPredictor.update_fn_guide (sampling.py:191-207: the EM step minus grad_step x the gradient of the masked
    Tweedie residual norm w.r.t. x_t, i.e. a backward pass THROUGH the score network to its input) on the HIP forward /
    input-gradient path vs the reference's own output (golden g16), sub-VP and VP, the golden's z injected.  The step runs inside
    ``model.input_grad_only()``: no weight-gradient GEMM is launched for it."""
    from dposer_amd.algorithms.advanced import sampling, sde_lib
    from dposer_amd.algorithms.advanced import utils as mutils
    g = load("g16_guided_step")
    cfg, m, p = make_model(int(g["seed"]), precision=prec)
    x_t, obs, mask = _dev(g["x_t"]), _dev(g["obs"]), _dev(g["mask"])
    for name, sde in (("subvp", sde_lib.subVPSDE(0.1, 20.0, 1000)), ("vp", sde_lib.VPSDE(0.1, 20.0, 1000))):
        score_fn = mutils.get_score_fn(sde, m, train=False, continuous=True)
        pred = sampling.EulerMaruyamaPredictor(sde, score_fn, probability_flow=False)
        for tv in (0.9, 0.3):
            tag = f"{name}_t{int(tv * 10)}"
            z = _dev(g[f"{tag}_z"])
            monkeypatch.setattr(torch, "randn_like", lambda x, **kw: z)
            y_hat, y_mean = pred.update_fn_guide(x_t.clone(), torch.ones(x_t.shape[0], device=DEV) * tv, obs, mask, grad_step=0.7)
            monkeypatch.undo()
            assert rel_err(t2n(y_mean), g[f"{tag}_y_mean"]) < tol, tag
            assert rel_err(t2n(y_hat), g[f"{tag}_y_hat"]) < tol, tag
    assert all(q.grad is None for q in m.parameters())


def test_langevin_corrector_fused_path_matches_reference_golden():
    """Langevin corrector + EM predictor (sampling.py:282-302, 182-188) on the HIP path -- dposer_langevin_step (two phases around
    the batch-mean norms) + dposer_em_sampler_steps -- fed the golden's recorded draws in the reference's order."""
    g = load("g5_sampler")
    cfg, m, p = make_model(int(g["seed"]), precision="fp32")
    sde, fn = _sampler(m, cfg, 1000, 16, corrector="langevin")
    noise = _dev(g["lang4_noise"]).reshape(4, 2, 16, 63)             # per step: corrector draw, predictor draw
    trajs, x = fn(m, z=_dev(g["lang4_z0"]), start_step=996, args=_Args("denoise"), noise=noise)
    assert rel_err(t2n(trajs), g["lang4_trajs"]) < 2e-5              # measured ~1e-6
    assert rel_err(t2n(x), g["lang4_final"]) < 2e-5


def test_langevin_generic_class_matches_reference_golden():
    """The generic LangevinCorrector / EulerMaruyamaPredictor classes (any score function) on the HIP score function; the torch
    RNG draws are replaced by the golden's recorded noise."""
    from unittest import mock
    from dposer_amd.algorithms.advanced import sampling
    g = load("g5_sampler")
    cfg, m, p = make_model(int(g["seed"]), precision="fp32")
    sde, _ = _sampler(m, cfg, 1000, 16, corrector="langevin")
    noise = iter(_dev(g["lang4_noise"]))
    x = _dev(g["lang4_z0"])
    ts = torch.linspace(sde.T, 1e-3, sde.N, device=DEV)
    trajs = []
    with torch.no_grad(), mock.patch.object(torch, "randn_like", lambda x, **k: next(noise)):
        for i in range(996, 1000):
            vec_t = torch.ones(16, device=DEV) * ts[i]
            x, _ = sampling.shared_corrector_update_fn(x, vec_t, None, None, sde, m, sampling.LangevinCorrector, True, cfg.sampling.snr, 1)
            x, xm = sampling.shared_predictor_update_fn(x, vec_t, None, None, sde, m, sampling.EulerMaruyamaPredictor, False, True)
            trajs.append(x)
    assert rel_err(t2n(torch.stack(trajs)), g["lang4_trajs"]) < 2e-4
    assert rel_err(t2n(xm), g["lang4_final"]) < 2e-4


def test_langevin_fused_inkernel_noise_vs_oracle():
    """No injected draws: corrector and predictor noise from Philox (two phases of a Langevin step regenerate the same numbers);
    the oracle gets them from oracle/philox.py.  (N = 1000: Langevin's alpha = 1 - beta_i / N needs a fine grid to stay positive.)"""
    cfg, m, p = make_model(23, precision="fp32")
    N, B, seed, start = 1000, 48, 99, 994
    sde, fn = _sampler(m, cfg, N, B, corrector="langevin")
    rs = np.random.RandomState(6)
    z0 = (rs.standard_normal((B, 63)) * 0.3).astype(np.float32)
    trajs, x = fn(m, z=_dev(z0), seed=seed, start_step=start, args=_Args("denoise"))
    xo = torch.tensor(z0)
    so = R.SubVP(N=N)
    ts = torch.linspace(1.0, 1e-3, N)
    for k, i in enumerate(range(start, N)):
        t = torch.ones(B) * ts[i]
        zc = torch.tensor(PH.normal_matrix(B, 63, PH.STREAM_LANGEVIN, i, seed))
        xo, _ = R.langevin_step(p, so, xo, t, zc, snr=cfg.sampling.snr)
        zp = torch.tensor(PH.normal_matrix(B, 63, PH.STREAM_EM_NOISE, i, seed))
        xo, xm = R.em_step(p, so, xo, t, zp)
        assert rel_err(t2n(trajs[k]), xo.numpy()) < 1e-4, i
    assert rel_err(t2n(x), xm.numpy()) < 1e-4


def test_em_sampler_1000_steps_golden():
    g = load("g5_sampler")
    cfg, m, p = make_model(int(g["seed"]), precision="fp32")
    sde, fn = _sampler(m, cfg, 1000, 8)
    rs = np.random.RandomState(int(g["em1000_noise_seed"]))
    noise = np.stack([rs.standard_normal((8, 63)).astype(np.float32) for _ in range(int(g["em1000_noise_count"]))])
    trajs, x = fn(m, z=_dev(g["em1000_z0"]), noise=_dev(noise)[:, None], traj_stride=100)
    assert trajs.shape == (10, 8, 63)
    assert rel_err(t2n(trajs), g["em1000_trajs"]) < 5e-3
    assert rel_err(t2n(x), g["em1000_final"]) < 5e-3


def test_em_sampler_inkernel_philox_matches_oracle():
    """No injected noise: the kernel draws Philox normals; the oracle is fed the same numbers from the numpy
    restatement of the RNG contract (oracle/philox.py)."""
    cfg, m, p = make_model(21, precision="fp32")
    N, B, seed = 6, 40, 777
    sde, fn = _sampler(m, cfg, N, B)
    rs = np.random.RandomState(3)
    z0 = rs.standard_normal((B, 63)).astype(np.float32)
    trajs, x = fn(m, z=_dev(z0), seed=seed)
    noises = [torch.tensor(PH.normal_matrix(B, 63, PH.STREAM_EM_NOISE, i, seed)) for i in range(N)]
    ref_trajs, ref_x = R.pc_sampler(p, R.SubVP(N=N), torch.tensor(z0), noises)
    assert rel_err(t2n(trajs), ref_trajs.numpy()) < 1e-4
    assert rel_err(t2n(x), ref_x.numpy()) < 1e-4
    trajs2, x2 = fn(m, z=_dev(z0), seed=seed)                   # same key -> bit-identical
    assert torch.equal(trajs, trajs2) and torch.equal(x, x2)
    trajs3, _ = fn(m, z=_dev(z0), seed=seed + 1)
    assert not torch.equal(trajs, trajs3)


@pytest.mark.parametrize("B,prec,tol", [(40, "fp32", 1e-4), (300, "fp32", 1e-4), (1000, "bf16", 1e-2), (300, "bf16x3", 1e-4)])      # bf16 measured 4.4e-3
def test_em_sampler_fused_step_path_matches_oracle(B, prec, tol):
    """traj_stride = 0 (no trajectory), no observation, in-kernel noise: post_dense and the Euler-Maruyama update run as one
    GEMM launch per step on an FT-resident state.  Must agree with the oracle fed the same Philox draws, return x_mean of the
    last step (noise_removal), and be bit-identical to the unfused path (same arithmetic, same counters) in fp32."""
    cfg, m, p = make_model(21, precision=prec)
    N, seed = 6, 4242
    sde, fn = _sampler(m, cfg, N, B)
    z0 = np.random.RandomState(B).standard_normal((B, 63)).astype(np.float32)
    trajs, x = fn(m, z=_dev(z0), seed=seed, traj_stride=0)
    assert trajs.shape[0] == 0 and x.shape == (B, 63)
    noises = [torch.tensor(PH.normal_matrix(B, 63, PH.STREAM_EM_NOISE, i, seed)) for i in range(N)]
    ref_trajs, ref_x = R.pc_sampler(p, R.SubVP(N=N), torch.tensor(z0), noises)
    assert rel_err(t2n(x), ref_x.numpy()) < tol
    trajs_u, x_u = fn(m, z=_dev(z0), seed=seed, traj_stride=1)                # unfused path keeps the trajectory
    if prec == "fp32":
        assert rel_err(t2n(x), t2n(x_u)) < 2e-6
    assert rel_err(t2n(trajs_u[-1]), ref_trajs[-1].numpy()) < tol


def test_inkernel_noise_statistics():
    cfg, m, p = make_model(22, precision="bf16")
    sde, fn = _sampler(m, cfg, 2, 8192)
    z0 = torch.zeros(8192, 63, device=DEV)
    trajs, _ = fn(m, z=z0, seed=5)
    z = PH.normal_matrix(8192, 63, PH.STREAM_EM_NOISE, 0, 5)
    assert abs(z.mean()) < 5e-3 and abs(z.std() - 1) < 5e-3
    assert torch.isfinite(trajs).all()


# ------------------------------------------------------------------------------------------------
# DPoser prior loss
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec,tol", [("fp32", 2e-4), ("bf16", 2e-3), ("bf16x3", 2e-4)])      # bf16 measured 3.4e-4 (gradient)
def test_prior_loss_matches_reference_golden(prec, tol):
    from dposer_amd.algorithms.advanced import sde_lib
    from dposer_amd.prior import prior_loss
    g = load("g7_prior_loss")
    cfg, m, p = make_model(int(g["seed"]), precision=prec)
    sde = sde_lib.subVPSDE(0.1, 20.0, 1000)
    for step in (0, 99, 100, 199):
        x0 = _dev(g["x0"]).requires_grad_(True)
        loss = prior_loss(m, sde, x0, float(g[f"s{step}_t"]), weighted=bool(int(g[f"s{step}_quan_t"])), z=_dev(g[f"s{step}_z"]))
        loss.backward()
        assert abs(float(loss) - float(g[f"s{step}_loss"])) / abs(float(g[f"s{step}_loss"])) < tol
        assert rel_err(t2n(x0.grad), g[f"s{step}_grad"]) < tol
        lu = prior_loss(m, sde, _dev(g["x0"]), float(g[f"s{step}_t"]), weighted=False, z=_dev(g[f"s{step}_z"]))
        assert abs(float(lu) - float(g[f"s{step}_loss_unweighted"])) / abs(float(g[f"s{step}_loss_unweighted"])) < tol


@pytest.mark.parametrize("prec,tol_loss,tol_grad,tol", [("fp32", 2e-5, 2e-4, 1e-4), ("bf16", 5e-3, 8e-3, 1e-2), ("bf16x3", 2e-5, 2e-4, 1e-4)])
def test_fourier_embedding_fused_paths_match_reference_golden(prec, tol_loss, tol_grad, tol, monkeypatch):
    """`config.model.embedding_type = 'fourier'` (the shipped config's documented alternative: GaussianFourierProjection of
    log(labels), output divided by the labels -- model.py:117-118,152-155) on the ONE-CALL paths: fused DSM step, fused EM sampler
    (plain and with completion imputation), prior loss and the completion loop, each against the reference's own output with its
    recorded draws (golden g20).  The fused entry points must be the ones that run: the step-by-step fallbacks are made to raise."""
    from dposer_amd.algorithms.advanced import sampling, sde_lib
    from dposer_amd.prior import prior_loss
    from dposer_amd.tasks.completion import DPoserComp
    g = load("g20_fourier_paths")
    cfg, m, p = make_model(int(g["seed"]), precision=prec, dropout=0.0, embedding="fourier")
    sde = sde_lib.subVPSDE(0.1, 20.0, 1000)
    assert sampling.fused_em_supported(sde, m, sampling.EulerMaruyamaPredictor, sampling.NoneCorrector, False, True)
    # DSM loss + every parameter gradient
    t = _dev(g["dsm_u"]) * (1.0 - 1e-5) + 1e-5
    loss, fg = _fused_grad(m, _dev(g["dsm_batch"]), t, _dev(g["dsm_z"]))
    assert abs(loss - float(g["dsm_loss"])) / float(g["dsm_loss"]) < tol_loss
    for (name, prm), off in zip(m.named_parameters(), m._offsets):
        ref = g[f"dsm_grad/{name}"]
        got = fg[off:off + prm.numel()]
        if ref.shape == (1,):
            assert float(got.abs().max()) == 0.0          # pre_dense_cond and the fixed projection W: no gradient
            continue
        assert rel_err(probe(name, got), ref) < tol_grad, name
    # EM sampler, N = 8: plain and with the completion imputation
    monkeypatch.setattr(sampling, "shared_predictor_update_fn", lambda *a, **k: (_ for _ in ()).throw(AssertionError("step-by-step sampler used")))
    cfg8, m8, _ = make_model(int(g["seed"]), precision=prec, embedding="fourier")
    sde8, fn = _sampler(m8, cfg8, 8, 16)
    trajs, x = fn(m8, z=_dev(g["em8_z0"]), noise=_dev(g["em8_noise"])[:, None])
    assert rel_err(t2n(trajs), g["em8_trajs"]) < tol and rel_err(t2n(x), g["em8_final"]) < tol
    trajs, x = fn(m8, observation=_dev(g["comp8_obs"]), mask=_dev(g["comp8_mask"]), z=_dev(g["comp8_z0"]), args=_Args("completion"),
                  noise=_dev(g["comp8_noise"]).reshape(8, 3, 16, 63))
    assert rel_err(t2n(trajs), g["comp8_trajs"]) < tol and rel_err(t2n(x), g["comp8_final"]) < tol
    # prior loss + its gradient
    for step in (0, 199):
        x0 = _dev(g["prior_x0"]).requires_grad_(True)
        lp = prior_loss(m8, sde, x0, float(g[f"prior_s{step}_t"]), weighted=bool(int(g[f"prior_s{step}_quan_t"])), z=_dev(g[f"prior_s{step}_z"]))
        lp.backward()
        assert abs(float(lp) - float(g[f"prior_s{step}_loss"])) / abs(float(g[f"prior_s{step}_loss"])) < max(tol, 2e-4)
        assert rel_err(t2n(x0.grad), g[f"prior_s{step}_grad"]) < max(tol, 2e-4)
    # the completion loop as one call
    comp = DPoserComp(m8, sde, continuous=True, batch_size=16)
    assert comp._fused_supported()
    out = comp.optimize(_dev(g["loop_observation"]), _dev(g["loop_mask"]), iterations=int(g["loop_iterations"]),
                        steps_per_iter=int(g["loop_steps_per_iter"]), noise=_dev(g["loop_noise"]))
    assert rel_err(t2n(out), g["loop_out"]) < max(tol, 2e-4)


@pytest.mark.parametrize("prec,tol_loss,tol_grad,tol", [("fp32", 2e-5, 2e-4, 1e-4), ("bf16", 1e-2, 2e-2, 2e-2), ("bf16x3", 2e-5, 2e-4, 1e-4)])
def test_ve_sde_fused_paths_match_reference_golden(prec, tol_loss, tol_grad, tol, monkeypatch):
    """The variance-exploding SDE (sde_lib.py:234-292; continuous score function utils.py:164-181: the network is conditioned on
    sigma(t) = sigma_min (sigma_max / sigma_min)^t and its output is the score) on the ONE-CALL paths -- fused DSM step, fused EM sampler
    (plain and with completion imputation), prior loss, completion loop -- against the reference's own outputs with its recorded draws
    (golden g21).  Rounds 1-4 ran VE step by step on the HIP score function; the fallbacks are made to raise here."""
    from dposer_amd.algorithms.advanced import sampling, sde_lib
    from dposer_amd.algorithms.advanced.losses import fused_dsm_grad, fused_dsm_supported
    from dposer_amd.prior import prior_loss
    from dposer_amd import prior as prior_mod
    from dposer_amd.tasks.completion import DPoserComp
    g = load("g21_ve_paths")
    mk = lambda N: sde_lib.VESDE(sigma_min=float(g["sigma_min"]), sigma_max=float(g["sigma_max"]), N=N)
    cfg, m, p = make_model(int(g["seed"]), precision=prec, dropout=0.0)
    sde = mk(1000)
    assert sampling.fused_em_supported(sde, m, sampling.EulerMaruyamaPredictor, sampling.NoneCorrector, False, True)
    assert sampling.fused_em_supported(sde, m, sampling.EulerMaruyamaPredictor, sampling.NoneCorrector, False, False)         # discrete VE: other labels, same kernels (g25)
    assert sampling.fused_em_supported(sde_lib.VPSDE(0.1, 20.0, 1000), m, sampling.EulerMaruyamaPredictor, sampling.NoneCorrector, False, False)         # discrete VP too (g26)
    assert fused_dsm_supported(sde, m, True, True, False, False)
    # DSM loss + every parameter gradient
    t = _dev(g["dsm_u"]) * (1.0 - 1e-5) + 1e-5
    fg = torch.zeros(m._num_flat, device=DEV)
    loss = float(fused_dsm_grad(m, sde, _dev(g["dsm_batch"]), flat_grad=fg, t=t, z=_dev(g["dsm_z"]), seed=m._rng_seed, step=0))
    assert abs(loss - float(g["dsm_loss"])) / float(g["dsm_loss"]) < tol_loss
    for (name, prm), off in zip(m.named_parameters(), m._offsets):
        ref = g[f"dsm_grad/{name}"]
        got = fg[off:off + prm.numel()]
        if ref.shape == (1,):
            assert float(got.abs().max()) == 0.0
            continue
        assert rel_err(probe(name, got), ref) < tol_grad, name
    # EM sampler, N = 8: plain and with the completion imputation
    monkeypatch.setattr(sampling, "shared_predictor_update_fn", lambda *a, **k: (_ for _ in ()).throw(AssertionError("step-by-step sampler used")))
    monkeypatch.setattr(prior_mod, "_prior_loss_unfused", lambda *a, **k: (_ for _ in ()).throw(AssertionError("step-by-step prior loss used")))
    cfg8, m8, _ = make_model(int(g["seed"]), precision=prec)
    cfg8.sampling.corrector = "none"
    fn = sampling.get_sampling_fn(cfg8, mk(8), (16, 63), lambda x: x, 1e-3, device=DEV)
    trajs, x = fn(m8, z=_dev(g["em8_z0"]), noise=_dev(g["em8_noise"])[:, None])
    assert rel_err(t2n(trajs), g["em8_trajs"]) < tol and rel_err(t2n(x), g["em8_final"]) < tol
    trajs, x = fn(m8, observation=_dev(g["comp8_obs"]), mask=_dev(g["comp8_mask"]), z=_dev(g["comp8_z0"]), args=_Args("completion"),
                  noise=_dev(g["comp8_noise"]).reshape(8, 3, 16, 63))
    assert rel_err(t2n(trajs), g["comp8_trajs"]) < tol and rel_err(t2n(x), g["comp8_final"]) < tol
    # prior loss + its gradient
    for step in (0, 199):
        x0 = _dev(g["prior_x0"]).requires_grad_(True)
        lp = prior_loss(m8, sde, x0, float(g[f"prior_s{step}_t"]), weighted=bool(int(g[f"prior_s{step}_quan_t"])), z=_dev(g[f"prior_s{step}_z"]))
        lp.backward()
        assert abs(float(lp) - float(g[f"prior_s{step}_loss"])) / abs(float(g[f"prior_s{step}_loss"])) < max(tol, 2e-4)
        assert rel_err(t2n(x0.grad), g[f"prior_s{step}_grad"]) < max(tol, 2e-4)
    # the completion loop as one call
    comp = DPoserComp(m8, sde, continuous=True, batch_size=16)
    assert comp._fused_supported()
    out = comp.optimize(_dev(g["loop_observation"]), _dev(g["loop_mask"]), iterations=int(g["loop_iterations"]),
                        steps_per_iter=int(g["loop_steps_per_iter"]), noise=_dev(g["loop_noise"]))
    assert rel_err(t2n(out), g["loop_out"]) < max(tol, 2e-4)


@pytest.mark.parametrize("prec,tol", [("fp32", 1e-4), ("bf16", 2e-2), ("bf16x3", 1e-4)])
def test_discrete_ve_score_function_on_the_fused_paths_matches_reference_golden(prec, tol, monkeypatch):
    """training.continuous = False under the VE SDE (get_score_fn(..., continuous=False), utils.py:175-181: the network is conditioned on the label
    round((T - t)(N - 1)) -- an index into `sigmas`, the argument of the positional embedding) on the one-call paths (DPOSER_SDE_VE_DISCRETE, round 6):
    EM sampler (plain and with completion imputation), prior loss + gradient, completion loop, against the reference's own outputs with its recorded
    draws (golden g25).  The step-by-step fallbacks are made to raise; the training step refuses the kind (a discrete model trains on the SMLD loss)."""
    from dposer_amd.algorithms.advanced import sampling, sde_lib
    from dposer_amd.algorithms.advanced.losses import fused_dsm_supported
    from dposer_amd.prior import prior_loss
    from dposer_amd import prior as prior_mod, _C
    from dposer_amd.tasks.completion import DPoserComp
    g = load("g25_ve_discrete_paths")
    mk = lambda N: sde_lib.VESDE(sigma_min=float(g["sigma_min"]), sigma_max=float(g["sigma_max"]), N=N)
    cfg8, m8, _ = make_model(int(g["seed"]), precision=prec)
    cfg8.training.continuous = False
    cfg8.sampling.corrector = "none"
    assert sde_lib.sde_desc(mk(8), False).kind == _C.SDE_VE_DISCRETE and sde_lib.sde_desc(mk(8)).kind == _C.SDE_VE
    assert not fused_dsm_supported(mk(1000), m8, False, True, False, False)
    monkeypatch.setattr(sampling, "shared_predictor_update_fn", lambda *a, **k: (_ for _ in ()).throw(AssertionError("step-by-step sampler used")))
    monkeypatch.setattr(prior_mod, "_prior_loss_unfused", lambda *a, **k: (_ for _ in ()).throw(AssertionError("step-by-step prior loss used")))
    fn = sampling.get_sampling_fn(cfg8, mk(8), (16, 63), lambda x: x, 1e-3, device=DEV)
    trajs, x = fn(m8, z=_dev(g["em8_z0"]), noise=_dev(g["em8_noise"])[:, None])
    assert rel_err(t2n(trajs), g["em8_trajs"]) < tol and rel_err(t2n(x), g["em8_final"]) < tol
    trajs, x = fn(m8, observation=_dev(g["comp8_obs"]), mask=_dev(g["comp8_mask"]), z=_dev(g["comp8_z0"]), args=_Args("completion"),
                  noise=_dev(g["comp8_noise"]).reshape(8, 3, 16, 63))
    assert rel_err(t2n(trajs), g["comp8_trajs"]) < tol and rel_err(t2n(x), g["comp8_final"]) < tol
    sde = mk(1000)
    for step in (0, 100, 199):
        x0 = _dev(g["prior_x0"]).requires_grad_(True)
        lp = prior_loss(m8, sde, x0, float(g[f"prior_s{step}_t"]), weighted=bool(int(g[f"prior_s{step}_quan_t"])), z=_dev(g[f"prior_s{step}_z"]),
                        continuous=False)
        lp.backward()
        assert abs(float(lp) - float(g[f"prior_s{step}_loss"])) / abs(float(g[f"prior_s{step}_loss"])) < max(tol, 2e-4)
        assert rel_err(t2n(x0.grad), g[f"prior_s{step}_grad"]) < max(tol, 2e-4)
    comp = DPoserComp(m8, sde, continuous=False, batch_size=16)
    assert comp._fused_supported()
    out = comp.optimize(_dev(g["loop_observation"]), _dev(g["loop_mask"]), iterations=int(g["loop_iterations"]),
                        steps_per_iter=int(g["loop_steps_per_iter"]), noise=_dev(g["loop_noise"]))
    assert rel_err(t2n(out), g["loop_out"]) < max(tol, 2e-4)
    # the continuous score function on the same inputs must NOT land on the discrete golden (the label really is another one)
    cfg8.training.continuous = True
    fn_c = sampling.get_sampling_fn(cfg8, mk(8), (16, 63), lambda x: x, 1e-3, device=DEV)
    _, xc = fn_c(m8, z=_dev(g["em8_z0"]), noise=_dev(g["em8_noise"])[:, None])
    assert rel_err(t2n(xc), g["em8_final"]) > 10 * tol


@pytest.mark.parametrize("prec,tol", [("fp32", 1e-4), ("bf16", 2e-2), ("bf16x3", 1e-4)])
def test_discrete_vp_score_function_on_the_fused_paths_matches_reference_golden(prec, tol, monkeypatch):
    """training.continuous = False under the VP SDE (get_score_fn(..., continuous=False), utils.py:157-162: label t (N - 1), score =
    -model / sqrt_1m_alphas_cumprod[label.long()], the DDPM table of sde_lib.py:134-139) on the one-call paths (DPOSER_SDE_VP_DISCRETE, round 6): EM
    sampler (plain and with completion imputation), prior loss + gradient, completion loop, against the reference's own outputs with its recorded
    draws (golden g26).  The step-by-step fallbacks are made to raise.  A VPSDE whose N was changed after construction keeps the constructor's
    table in the reference: such an object stays off the fused paths."""
    from dposer_amd.algorithms.advanced import sampling, sde_lib
    from dposer_amd.algorithms.advanced.losses import fused_dsm_supported
    from dposer_amd.prior import prior_loss
    from dposer_amd import prior as prior_mod, _C
    from dposer_amd.tasks.completion import DPoserComp
    g = load("g26_vp_discrete_paths")
    mk = lambda N: sde_lib.VPSDE(beta_min=float(g["beta_min"]), beta_max=float(g["beta_max"]), N=N)
    cfg8, m8, _ = make_model(int(g["seed"]), precision=prec)
    cfg8.training.continuous = False
    cfg8.sampling.corrector = "none"
    assert sde_lib.sde_desc(mk(8), False).kind == _C.SDE_VP_DISCRETE and sde_lib.sde_desc(mk(8)).kind == _C.SDE_VP
    stale = mk(1000)
    stale.N = 500
    assert sde_lib.sde_desc(stale, False) is None and sde_lib.sde_desc(stale) is not None
    assert not fused_dsm_supported(mk(1000), m8, False, True, False, False)
    monkeypatch.setattr(sampling, "shared_predictor_update_fn", lambda *a, **k: (_ for _ in ()).throw(AssertionError("step-by-step sampler used")))
    monkeypatch.setattr(prior_mod, "_prior_loss_unfused", lambda *a, **k: (_ for _ in ()).throw(AssertionError("step-by-step prior loss used")))
    fn = sampling.get_sampling_fn(cfg8, mk(8), (16, 63), lambda x: x, 1e-3, device=DEV)
    trajs, x = fn(m8, z=_dev(g["em8_z0"]), noise=_dev(g["em8_noise"])[:, None])
    assert rel_err(t2n(trajs), g["em8_trajs"]) < tol and rel_err(t2n(x), g["em8_final"]) < tol
    trajs, x = fn(m8, observation=_dev(g["comp8_obs"]), mask=_dev(g["comp8_mask"]), z=_dev(g["comp8_z0"]), args=_Args("completion"),
                  noise=_dev(g["comp8_noise"]).reshape(8, 3, 16, 63))
    assert rel_err(t2n(trajs), g["comp8_trajs"]) < tol and rel_err(t2n(x), g["comp8_final"]) < tol
    sde = mk(1000)
    for step in (0, 100, 199):
        x0 = _dev(g["prior_x0"]).requires_grad_(True)
        lp = prior_loss(m8, sde, x0, float(g[f"prior_s{step}_t"]), weighted=bool(int(g[f"prior_s{step}_quan_t"])), z=_dev(g[f"prior_s{step}_z"]),
                        continuous=False)
        lp.backward()
        assert abs(float(lp) - float(g[f"prior_s{step}_loss"])) / abs(float(g[f"prior_s{step}_loss"])) < max(tol, 2e-4)
        assert rel_err(t2n(x0.grad), g[f"prior_s{step}_grad"]) < max(tol, 2e-4)
    comp = DPoserComp(m8, sde, continuous=False, batch_size=16)
    assert comp._fused_supported()
    out = comp.optimize(_dev(g["loop_observation"]), _dev(g["loop_mask"]), iterations=int(g["loop_iterations"]),
                        steps_per_iter=int(g["loop_steps_per_iter"]), noise=_dev(g["loop_noise"]))
    assert rel_err(t2n(out), g["loop_out"]) < max(tol, 2e-4)
    # the continuous score function on the same inputs must NOT land on the discrete golden (the label really is another one)
    cfg8.training.continuous = True
    fn_c = sampling.get_sampling_fn(cfg8, mk(8), (16, 63), lambda x: x, 1e-3, device=DEV)
    _, xc = fn_c(m8, z=_dev(g["em8_z0"]), noise=_dev(g["em8_noise"])[:, None])
    assert rel_err(t2n(xc), g["em8_final"]) > 10 * tol


# ------------------------------------------------------------------------------------------------
# training: DSM loss, gradients, Adam / EMA
# ------------------------------------------------------------------------------------------------
def _fused_grad(m, batch, t, z, step=0):
    from dposer_amd.algorithms.advanced import sde_lib
    from dposer_amd.algorithms.advanced.losses import fused_dsm_grad
    fg = torch.zeros(m._num_flat, device=DEV)
    loss = fused_dsm_grad(m, sde_lib.subVPSDE(0.1, 20.0, 1000), batch, flat_grad=fg, t=t, z=z, seed=m._rng_seed, step=step)
    return float(loss), fg


@pytest.mark.parametrize("prec,tol_loss,tol_grad", [("fp32", 2e-5, 2e-4), ("bf16", 5e-3, 5e-3), ("bf16x3", 2e-5, 2e-4)])      # bf16 gradients measured 1.9e-3
def test_dsm_loss_and_grads_match_reference_golden(prec, tol_loss, tol_grad):
    g = load("g3_loss_grads")
    cfg, m, p = make_model(int(g["seed"]), precision=prec, dropout=0.0)
    batch = _dev(g["nodrop_batch"])
    t = _dev(g["nodrop_u"]) * (1.0 - 1e-5) + 1e-5
    loss, fg = _fused_grad(m, batch, t, _dev(g["nodrop_z"]))
    assert abs(loss - float(g["nodrop_loss"])) / float(g["nodrop_loss"]) < tol_loss
    for (name, prm), off in zip(m.named_parameters(), m._offsets):
        ref = g[f"nodrop_grad/{name}"]
        got = fg[off:off + prm.numel()]
        if ref.shape == (1,):
            assert float(got.abs().max()) == 0.0          # pre_dense_cond: no gradient
            continue
        assert rel_err(probe(name, got), ref) < tol_grad, name


@pytest.mark.parametrize("drop_p", [0.1, 0.5])
def test_dsm_with_inkernel_dropout_and_rng_matches_oracle(drop_p):
    """Dropout masks, t and z all drawn in-kernel (Philox); the oracle gets the same draws from oracle/philox.py."""
    cfg, m, p = make_model(31, precision="fp32", dropout=drop_p)
    B, step = 96, 7
    rs = np.random.RandomState(1)
    batch = rs.standard_normal((B, 63)).astype(np.float32)
    loss, fg = _fused_grad(m, _dev(batch), None, None, step=step)
    seed = m._rng_seed
    t = torch.tensor(PH.uniform_t(B, step, seed))
    z = torch.tensor(PH.normal_matrix(B, 63, PH.STREAM_TRAIN_Z, step, seed))
    masks = [torch.tensor(PH.dropout_keep_mask(B, 1024, site, step, seed, drop_p)) for site in range(5)]
    names = R.param_names()
    leaves = {n: p[n].clone().requires_grad_(True) for n in names}
    full = dict(p)
    full.update(leaves)
    ref = R.dsm_loss(full, R.SubVP(), torch.tensor(batch), t, z, drop_masks=masks, drop_p=drop_p)
    grads = torch.autograd.grad(ref, [leaves[n] for n in names], allow_unused=True)
    assert abs(loss - ref.item()) / ref.item() < 5e-5
    for n, gr, off in zip(names, grads, m._offsets):
        if gr is None:
            continue
        assert rel_err(t2n(fg[off:off + gr.numel()]), gr.reshape(-1).numpy()) < 3e-4, n


@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
def test_train_steps_match_reference_golden(prec):
    """step_fn (fused DSM + clip + Adam + EMA) against the reference's recorded steps 0,1,2,4999,5000.
    The reference ran with torch-RNG dropout masks that a kernel cannot reproduce -> dropout off here and the
    oracle (pinned to the same golden by tests/test_oracle_golden.py) is the arbiter for the dropout-free run."""
    from dposer_amd.algorithms.advanced import losses, sde_lib
    from dposer_amd.algorithms.ema import ExponentialMovingAverage
    g = load("g4_train_steps")
    cfg, m, p = make_model(int(g["seed"]), precision=prec, dropout=0.0)
    sde = sde_lib.subVPSDE(0.1, 20.0, 1000)
    opt = losses.get_optimizer(cfg, m.parameters())
    ema = ExponentialMovingAverage(m.parameters(), decay=cfg.model.ema_rate)
    state = dict(optimizer=opt, model=m, ema=ema, step=0)
    step_fn = losses.get_step_fn(sde, train=True, optimize_fn=losses.optimization_manager(cfg), reduce_mean=True, continuous=True)
    names = R.param_names()
    st = R.TrainState(p, names)
    batch = g["batch"]
    for i in range(5):
        s = int(g[f"s{i}_step"])
        state["step"] = s
        st.step = s
        t = torch.tensor(g[f"s{i}_u"]) * (1.0 - 1e-5) + 1e-5
        z = torch.tensor(g[f"s{i}_z"])
        out = step_fn(state, _dev(batch), t=t.to(DEV), z=z.to(DEV))
        ref_loss, _, _ = R.train_step(st, R.SubVP(), torch.tensor(batch), t, z)
        assert abs(float(out["step_loss"]) - ref_loss.item()) / ref_loss.item() < 5e-5
        assert abs(opt.param_groups[0]["lr"] - float(g[f"s{i}_lr"])) < 1e-12
        assert state["step"] == s + 1
        for (n, prm), off in zip(m.named_parameters(), m._offsets):
            assert rel_err(t2n(prm), st.p[n].numpy()) < 2e-5, (i, n)
            assert rel_err(t2n(ema.shadow_params[names.index(n)]), st.ema[n].numpy()) < 2e-5, (i, n)
            if n.startswith("pre_dense_cond"):
                continue
            assert rel_err(t2n(opt.state[prm]["exp_avg"]), st.m[n].numpy()) < 2e-4, (i, n)
            assert rel_err(t2n(opt.state[prm]["exp_avg_sq"]), st.v[n].numpy()) < 2e-4, (i, n)
    assert ema.num_updates == 5


@pytest.mark.parametrize("prec", ["fp32", "bf16", "bf16x3"])
def test_autograd_forward_backward_vs_oracle(prec):
    # bf16: the file's bf16 bounds -- TOL_BF16 forward, 2e-2 for a gradient through the network (measured 4.7e-3 forward, 7.1e-3 x.grad, at most 7.3e-3 a parameter);
    # tests/test_gpu_bf16_faithful.py holds the same path row by row to the rounding-faithful oracle
    tol_out, tol_dx, tol_dw = (TOL_BF16, 2e-2, 2e-2) if prec == "bf16" else (TOL_FP32, 2e-4, 3e-4)
    cfg, m, p = make_model(41, precision=prec, dropout=0.0)
    B = 50
    rs = np.random.RandomState(2)
    x = rs.standard_normal((B, 63)).astype(np.float32)
    t = rs.uniform(1e-3, 1, B).astype(np.float32)
    w = rs.standard_normal((B, 63)).astype(np.float32)
    xd = _dev(x).requires_grad_(True)
    out = m(xd, _dev(t) * 999)
    (out * _dev(w)).sum().backward()
    names = R.param_names()
    leaves = {n: p[n].clone().requires_grad_(True) for n in names}
    full = dict(p)
    full.update(leaves)
    xr = torch.tensor(x, requires_grad=True)
    ref = R.scorefc_forward(full, xr, torch.tensor(t) * 999)
    grads = torch.autograd.grad((ref * torch.tensor(w)).sum(), [xr] + [leaves[n] for n in names], allow_unused=True)
    assert rel_err(t2n(out), ref.detach().numpy()) < tol_out
    assert rel_err(t2n(xd.grad), grads[0].numpy()) < tol_dx
    for (n, prm), gr in zip(m.named_parameters(), grads[1:]):
        if gr is None:
            assert prm.grad is None
            continue
        assert rel_err(t2n(prm.grad), gr.numpy()) < tol_dw, n


def test_full_batch_train_step_properties():
    """BASELINE size (B = 65536): finite loss / gradient, pre_dense_cond untouched, and the gradient is the mean of
    the gradients of the two half batches (linearity of the batch mean) -- bf16 throughput mode."""
    cfg, m, p = make_model(51, precision="bf16", dropout=0.0)
    B = 65536
    gen = torch.Generator(device=DEV).manual_seed(3)
    batch = torch.randn(B, 63, device=DEV, generator=gen)
    t = torch.rand(B, device=DEV, generator=gen) * (1 - 1e-5) + 1e-5
    z = torch.randn(B, 63, device=DEV, generator=gen)
    loss, fg = _fused_grad(m, batch, t, z)
    h = B // 2
    l1, g1 = _fused_grad(m, batch[:h].contiguous(), t[:h].contiguous(), z[:h].contiguous())
    l2, g2 = _fused_grad(m, batch[h:].contiguous(), t[h:].contiguous(), z[h:].contiguous())
    assert np.isfinite(loss) and torch.isfinite(fg).all()
    assert abs(loss - 0.5 * (l1 + l2)) / loss < 1e-4
    assert rel_err(t2n(fg), t2n(0.5 * (g1 + g2))) < 2e-3
    lo, hi = m._engine().nograd[0]
    assert float(fg[lo:hi].abs().max()) == 0.0


@pytest.mark.parametrize("driver", ["device", "scipy"])
def test_likelihood_matches_reference_golden(driver):
    """get_likelihood_fn (probability-flow ODE + Hutchinson divergence through the HIP forward / input-gradient) against the
    reference's CPU run with the same injected epsilon, with the device-resident RK45 driver (ode_device.py: scipy's controller,
    state on the GPU) and with scipy itself.  The adaptive RK45 amplifies rounding differences through its step-size
    decisions, hence the looser bound than a single forward."""
    from dposer_amd.algorithms.advanced import likelihood, sde_lib
    g = load("g12_likelihood_ode")
    cfg, m, p = make_model(int(g["seed"]), precision="fp32")
    sde = sde_lib.subVPSDE(beta_min=0.1, beta_max=20.0, N=1000)
    data = _dev(g["data"])
    for kind in ("Rademacher", "Gaussian"):
        fn = likelihood.get_likelihood_fn(sde, lambda v: v, hutchinson_type=kind, rtol=1e-4, atol=1e-4, eps=1e-4, driver=driver)
        bpd, z, nfe = fn(m, data, epsilon=_dev(g[f"lik_{kind}/eps"]))
        # measured (round 3, one evaluation per right-hand side): Rademacher bpd 1.2e-5 / z 9.3e-6, Gaussian 1.5e-3 / 8.1e-4 (the
        # Gaussian probe vector weights the random-weight Jacobian's rounding far more); nfe 746 / 734 = the reference's counts
        tol = 1e-4 if kind == "Rademacher" else 4e-3
        assert rel_err(t2n(bpd), g[f"lik_{kind}/bpd"]) < tol, kind
        assert rel_err(t2n(z), g[f"lik_{kind}/z"]) < tol, kind
        assert abs(int(nfe) - int(g[f"lik_{kind}/nfe"])) <= 6, (kind, nfe)        # at most one RK45 step apart (6 evaluations)
    # the noise draw itself: +-1 entries
    eps = likelihood.hutchinson_noise(data, "Rademacher")
    assert set(np.unique(t2n(eps)).tolist()) <= {-1.0, 1.0}
    with pytest.raises(NotImplementedError):
        likelihood.hutchinson_noise(data, "uniform")


def test_device_and_scipy_ode_drivers_agree():
    """Same right-hand side (the HIP forward), same controller: the device-resident driver and scipy.integrate.solve_ivp make the
    same step decisions (identical nfe) and end on the same samples."""
    from dposer_amd.algorithms.advanced import sampling, sde_lib
    g = load("g12_likelihood_ode")
    cfg, m, p = make_model(int(g["seed"]), precision="fp32")
    sde = sde_lib.subVPSDE(beta_min=0.1, beta_max=20.0, N=1000)
    out = {}
    for driver in ("device", "scipy"):
        fn = sampling.get_ode_sampler(sde, (6, 63), lambda v: v, rtol=1e-4, atol=1e-4, eps=1e-3, device=DEV, driver=driver)
        out[driver] = fn(m, z=_dev(g["ode/z"]))
    assert out["device"][0] == out["scipy"][0]
    assert rel_err(t2n(out["device"][1]), t2n(out["scipy"][1])) < 1e-6


@pytest.mark.parametrize("driver", ["device", "scipy"])
def test_ode_sampler_matches_reference_golden(driver):
    from dposer_amd.algorithms.advanced import sampling, sde_lib
    g = load("g12_likelihood_ode")
    cfg, m, p = make_model(int(g["seed"]), precision="fp32")
    sde = sde_lib.subVPSDE(beta_min=0.1, beta_max=20.0, N=1000)
    for denoise in (0, 1):
        fn = sampling.get_ode_sampler(sde, (6, 63), lambda v: v, denoise=bool(denoise), rtol=1e-4, atol=1e-4, eps=1e-3, device=DEV,
                                      driver=driver)
        nfe, x = fn(m, z=_dev(g["ode/z"]))
        # random weights are not a trained score: the flow expands |x| by four orders of magnitude, and rounding differences with it
        assert rel_err(t2n(x), g[f"ode/x_denoise{denoise}"]) < 2e-3                  # measured 8.9e-5
        assert abs(int(nfe) - int(g[f"ode/nfe_denoise{denoise}"])) <= 24, nfe          # measured 434 vs 446: two RK45 steps
    cfg.sampling.method = "ode"
    assert callable(sampling.get_sampling_fn(cfg, sde, (6, 63), lambda v: v, 1e-3, device=DEV))


@pytest.mark.parametrize("B,D", [(1, 63), (63, 63), (65, 63), (300, 63), (1000, 63), (130, 126)])
def test_dsm_grads_ragged_batches_and_rot6d_vs_oracle(B, D):
    """Batches that are not multiples of the 64 / 256-sample padding (padded rows must contribute nothing to the loss, the
    GroupNorm partial sums or the weight gradients), a single sample, and the rot6d data dimension (D = 126)."""
    cfg, m, p = make_model(17, D=D, precision="fp32", dropout=0.0)
    rs = np.random.RandomState(B)
    batch = rs.standard_normal((B, D)).astype(np.float32)
    t = rs.uniform(1e-3, 1.0, B).astype(np.float32)
    z = rs.standard_normal((B, D)).astype(np.float32)
    loss, fg = _fused_grad(m, _dev(batch), _dev(t), _dev(z))
    names = R.param_names()
    leaves = {n: p[n].clone().requires_grad_(True) for n in names}
    full = dict(p)
    full.update(leaves)
    ref = R.dsm_loss(full, R.SubVP(), torch.tensor(batch), torch.tensor(t), torch.tensor(z))
    grads = torch.autograd.grad(ref, [leaves[n] for n in names], allow_unused=True)
    assert abs(loss - ref.item()) / ref.item() < 5e-5
    for n, gr, off in zip(names, grads, m._offsets):
        got = fg[off:off + p[n].numel()]
        if gr is None:
            assert float(got.abs().max()) == 0.0, n
            continue
        assert rel_err(t2n(got), gr.reshape(-1).numpy()) < 3e-4, (n, B)


def test_checkpoint_round_trip_in_reference_format(tmp_path):
    """run/train.py:395-403 saves {'model_state_dict', 'optimizer_state_dict', 'ema', 'step'}; run/train.py:186-190 restores
    them.  A run resumed from such a file must continue bit-identically, and a state dict produced by torch.optim.Adam itself
    (what a reference checkpoint holds) must load into the fused optimizer."""
    from dposer_amd.algorithms.advanced import losses, sde_lib
    from dposer_amd.algorithms.ema import ExponentialMovingAverage

    def build():
        cfg, m, p = make_model(23, precision="fp32", dropout=0.0)
        cfg.optim.warmup = 2
        opt = losses.get_optimizer(cfg, m.parameters())
        ema = ExponentialMovingAverage(m.parameters(), decay=cfg.model.ema_rate)
        fn = losses.get_step_fn(sde_lib.subVPSDE(0.1, 20.0, 1000), True, optimize_fn=losses.optimization_manager(cfg), reduce_mean=True,
                                continuous=True)
        return cfg, m, dict(model=m, optimizer=opt, ema=ema, step=0), fn

    rs = np.random.RandomState(8)
    data = [(_dev(rs.standard_normal((64, 63)).astype(np.float32)), _dev(rs.uniform(1e-3, 1, 64).astype(np.float32)),
             _dev(rs.standard_normal((64, 63)).astype(np.float32))) for _ in range(4)]
    cfg, m, state, fn = build()
    for b, t, z in data[:2]:
        fn(state, b, t=t, z=z)
    path = tmp_path / "checkpoint-step2.pth"
    torch.save({"epoch": 1, "model_state_dict": m.state_dict(), "optimizer_state_dict": state["optimizer"].state_dict(),
                "ema": state["ema"].state_dict(), "step": state["step"]}, path)
    for b, t, z in data[2:]:
        fn(state, b, t=t, z=z)

    cfg2, m2, state2, fn2 = build()
    ck = torch.load(path, map_location=DEV, weights_only=False)
    m2.load_state_dict(ck["model_state_dict"])
    state2["optimizer"].load_state_dict(ck["optimizer_state_dict"])
    state2["ema"].load_state_dict(ck["ema"])
    state2["step"] = ck["step"]
    for b, t, z in data[2:]:
        fn2(state2, b, t=t, z=z)
    assert torch.equal(m.flat_params(), m2.flat_params())
    assert all(torch.equal(a, b) for a, b in zip(state["ema"].shadow_params, state2["ema"].shadow_params))
    assert state2["step"] == 4 and state2["ema"].num_updates == state["ema"].num_updates

    # a plain torch.optim.Adam state dict (reference checkpoints) -> FusedAdam
    ref_params = [torch.nn.Parameter(q.detach().clone()) for q in m.parameters()]
    ref_opt = torch.optim.Adam(ref_params, lr=2e-4, betas=(0.9, 0.999), eps=1e-8)
    for q in ref_params:
        q.grad = torch.full_like(q, 1e-3)
    ref_opt.step()
    cfg3, m3, state3, fn3 = build()
    state3["optimizer"].load_state_dict(ref_opt.state_dict())
    flat, offs, params = state3["optimizer"]._ensure_flat()
    for q, o in zip(ref_params, offs):
        st = ref_opt.state[q]
        assert torch.equal(state3["optimizer"]._flat_m[o:o + q.numel()], st["exp_avg"].reshape(-1))
        assert torch.equal(state3["optimizer"]._flat_v[o:o + q.numel()], st["exp_avg_sq"].reshape(-1))
    assert state3["optimizer"]._step_count == 1


def test_integration_md_ctypes_stub_runs():
    """INTEGRATION.md section 3 shows the ctypes stub a reference maintainer would write against include/dposer_hip.h; the
    snippet is executed as written and must reproduce the module's forward."""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "INTEGRATION.md")).read()
    code = re.search(r"```python\n(import ctypes as C, math, torch\n.*?)```", src, re.S).group(1)
    ns = {}
    cwd = os.getcwd()
    os.chdir(root)                      # the snippet loads "dposer_amd/libdposer_hip.so" relative to the checkout
    try:
        exec(code, ns)
        cfg, m, p = make_model(5, precision="bf16")
        x = torch.randn(100, 63, device=DEV)
        labels = torch.rand(100, device=DEV) * 999
        out = ns["scorefc_forward"](m, x, labels)
    finally:
        os.chdir(cwd)
    with torch.no_grad():
        assert torch.equal(out, m(x, labels))


@pytest.mark.parametrize("env", [
    # 256x256 tilings from 256 samples up (DPOSER_SMALL_TILE_MAX / DPOSER_FINAL_SMALL_MAX = 0: nothing keeps a small batch on 128x32 / 64x32)
    {"DPOSER_GNBWD_BIG": "1", "DPOSER_WGRAD_BIG": "1", "DPOSER_BIG_MIN_BATCH": "256", "DPOSER_WGRAD_BATCHED": "0",
     "DPOSER_SMALL_TILE_MAX": "0", "DPOSER_FINAL_SMALL_MAX": "0"},
    # 128x128 everywhere, single stream
    {"DPOSER_GNBWD_BIG": "0", "DPOSER_WGRAD_BIG": "0", "DPOSER_WGRAD_STREAM": "0", "DPOSER_WGRAD_BATCHED": "0",
     "DPOSER_SMALL_TILE_MAX": "0", "DPOSER_FINAL_SMALL_MAX": "0"},
    {"DPOSER_WGRAD_TR": "0"},                                                                # bf16 wgrads on transposed copies
    {"DPOSER_WGRAD_STREAM": "1", "DPOSER_WGRAD_BATCHED": "0"},                                                  # wgrads on the second stream (default 8192..16384)
    {"DPOSER_WGRAD_BATCHED": "1"},                                                           # all 256x256 wgrad tiles in one launch (the single-GPU default)
])
def test_alternative_tilings_and_streams_keep_parity(env, tuning_env):
    """The tiling / stream policy depends on the batch size (256x256 GroupNorm-backward and wgrad tiles from 32768 samples,
    second stream up to 16384).  The policies are read once per process, so the gradient-parity tests are re-run in a child
    process with each policy forced onto the small batches the oracle can check.  That the first two environments force the tiling
    they name is asserted here, through dposer_scorefc_plan, before the child starts."""
    import os
    import subprocess
    import sys
    if os.environ.get("DPOSER_TILING_CHILD"):
        pytest.skip("child process")
    if "DPOSER_SMALL_TILE_MAX" in env:
        import score_plan as SP
        from dposer_amd import _C
        tile = SP.BIG if env["DPOSER_GNBWD_BIG"] == "1" else SP.MID
        tuning_env(**env)
        for prec in ("fp32", "bf16", "bf16x3"):
            h = SP.make_handle(1024, prec)
            try:
                assert SP.plan(h, 1000)[:8] == (1024, tile, tile, tile, SP.FINAL, tile, SP.SPLIT_K, 0), (prec, SP.plan(h, 1000))
                assert SP.plan(h, 65)[:5] == (128, SP.MID, SP.MID, SP.MID, SP.FINAL), (prec, SP.plan(h, 65))      # (128 samples: no 256-row tile)
            finally:
                _C.lib().dposer_scorefc_destroy(h)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    child_env = dict(os.environ, DPOSER_TILING_CHILD="1", **env)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_gpu_score.py"), "-m", "gpu", "-q", "-x", "-k",
                        "ragged_batches_and_rot6d or dsm_loss_and_grads or train_steps_match or autograd_forward_backward"],
                       cwd=root, env=child_env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout


@pytest.mark.parametrize("B,prec", [(1280, "bf16"), (300, "bf16"), (2048, "bf16"), (1280, "fp32")])      # (300: the 128 x 32 tiling keeps the one launch)
def test_layer_split_time_branch_dgrad_matches_the_one_launch_form(B, prec, tuning_env):
    """Up to 2048 samples the time-branch dgrad (dU = sum_l dy_l Wt_l, times act'(u)) runs one k-split per layer segment plus a
    reduce pass (k_silu_bwd_reduce) instead of one launch whose few tiles walk K = 5 x 1024 alone: the same products, the five
    layers' sums added at the end instead of inside one accumulator -- every gradient agrees to fp32 summation error, the ones
    that do not depend on dU bit for bit."""
    cfg, m, p = make_model(14, precision=prec, dropout=0.1)
    m.train()
    rs = np.random.RandomState(6)
    batch = _dev(rs.standard_normal((B, 63)).astype(np.float32))
    out = {}
    for cap in ("2048", "0"):
        tuning_env(DPOSER_SILU_SPLIT_MAX=cap)
        out[cap] = _fused_grad(m, batch, None, None, step=5)
    (l1, g1), (l0, g0) = out["2048"], out["0"]
    assert l1 == l0
    names = [n for n, _ in m.named_parameters()]
    for name, off, prm in zip(names, m._offsets, m.parameters()):
        a, b = g1[off:off + prm.numel()], g0[off:off + prm.numel()]
        if name.startswith("shared_time_embed"):
            assert rel_err(t2n(a), t2n(b)) < (2e-6 if prec == "fp32" else 2e-3), name     # bf16: dU is rounded to bf16 after the sum
        else:
            assert torch.equal(a, b), name


@pytest.mark.parametrize("B", [8192, 5000, 32768])
def test_batched_weight_gradient_launch_matches_the_per_layer_launches(B, tuning_env):
    """One launch for every 256x256 weight-gradient tile of the step (wgrad_batch.h: 16 lanes x 16 workgroups over a line of lane
    problems, partial tiles reduced in a fixed order) against two split-K launches per layer: same products, another partition of the
    sample sum -- the flat gradients agree to fp32 summation error, and the batched form is deterministic."""
    from dposer_amd.algorithms.advanced import losses, sde_lib
    cfg, m, p = make_model(5, precision="bf16")
    sde = sde_lib.subVPSDE(0.1, 20.0, 1000)
    rs = np.random.RandomState(11)
    x = _dev(rs.standard_normal((B, 63)).astype(np.float32))
    grads = {}
    for tag, flag in (("per-layer", "0"), ("batched", "1"), ("batched-again", "1")):
        tuning_env(DPOSER_WGRAD_BATCHED=flag)
        fg = torch.full((m._engine().num_params,), float("nan"), device=DEV)
        loss = losses.fused_dsm_grad(m, sde, x, flat_grad=fg, seed=3, step=7)
        grads[tag] = (fg.clone(), float(loss))
    assert torch.isfinite(grads["batched"][0]).all()
    assert torch.equal(grads["batched"][0], grads["batched-again"][0])
    assert not torch.equal(grads["batched"][0], grads["per-layer"][0])          # (another summation order: the batched path did run)
    assert grads["batched"][1] == grads["per-layer"][1]
    a, b = grads["batched"][0].double(), grads["per-layer"][0].double()
    assert float((a - b).norm() / b.norm()) < 2e-6
    eng = m._engine()
    for off, prm in zip(eng.offsets, m._param_list):          # every tensor on its own: a misplaced tile cannot hide behind the big ones
        sl = slice(off, off + prm.numel())
        if float(b[sl].norm()) > 0:
            assert float((a[sl] - b[sl]).norm() / b[sl].norm()) < 2e-5, off


@pytest.mark.parametrize("B,extra,D", [(640, {}, 63), (1024, {"DPOSER_WGRAD_BIG": "1"}, 63), (96, {}, 63), (1500, {}, 63),
                                       (2304, {"DPOSER_WGRAD_BIG": "1"}, 63), (320, {}, 147), (320, {}, 126), (320, {}, 336)])
def test_sample_major_wgrad_is_bit_identical_to_transposed_copy_path(B, extra, D, tmp_path):
    """bf16 weight gradients: the kernel that reads sample-major operands through transposing LDS reads (gemm_wgrad_tr.h,
    default) and the plain kernel on transposed activation copies (DPOSER_WGRAD_TR=0, child process) accumulate in the same
    order -- the flat gradient must agree bit for bit, for the 128x128 / 64x128 / 128x64 tilings and (forced) 256x256."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = (
        "import sys, os, numpy as np, torch\n"
        f"sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, 'tests')); sys.path.insert(0, os.path.join({root!r}, 'tests', 'golden'))\n"
        "from gpu_common import make_model\n"
        "from test_gpu_score import _fused_grad, _dev\n"
        f"cfg, m, p = make_model(5, D={D}, precision='bf16', dropout=0.1)\n"
        f"rs = np.random.RandomState(3); batch = rs.standard_normal(({B}, {D})).astype(np.float32)\n"
        "loss, fg = _fused_grad(m, _dev(batch), None, None, step=11)\n"
        "np.save(sys.argv[1], fg.detach().cpu().numpy())\n")
    outs = []
    for tr in ("1", "0"):
        out = str(tmp_path / f"fg_tr{tr}.npy")
        # (per-layer launches on both sides: the one-launch form of wgrad_batch.h partitions the sample sum differently; the one-launch
        #  time-branch dgrad on both sides: its layer-split form -- sample-major mode only -- adds the layers' sums in another order)
        env = dict(os.environ, DPOSER_WGRAD_TR=tr, DPOSER_WGRAD_BATCHED="0", DPOSER_SILU_SPLIT_MAX="0", **extra)
        r = subprocess.run([sys.executable, "-c", code, out], cwd=root, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        outs.append(np.load(out))
    assert np.isfinite(outs[0]).all() and np.abs(outs[0]).max() > 0
    assert np.array_equal(outs[0], outs[1])


@pytest.mark.parametrize("B", [8193, 16385, 32769])
def test_gradient_is_linear_in_the_batch_across_tiling_thresholds(B):
    """Size-independent property at the batch sizes where the tiling / stream policies switch (padded to 8448, 16640, 33024
    samples; bf16, dropout off, injected t and z): loss and flat gradient of the whole batch equal the sample-weighted
    combination of two uneven halves evaluated separately (which take other tilings)."""
    cfg, m, p = make_model(5, precision="bf16", dropout=0.0)
    rs = np.random.RandomState(B)
    x = rs.standard_normal((B, 63)).astype(np.float32)
    t = rs.uniform(1e-3, 1.0, B).astype(np.float32)
    z = rs.standard_normal((B, 63)).astype(np.float32)
    l, g = _fused_grad(m, _dev(x), _dev(t), _dev(z))
    g = g.clone()
    h = B // 2 + 7
    l1, g1 = _fused_grad(m, _dev(x[:h]), _dev(t[:h]), _dev(z[:h]))
    g1 = g1.clone()
    l2, g2 = _fused_grad(m, _dev(x[h:]), _dev(t[h:]), _dev(z[h:]))
    gc = (h * g1 + (B - h) * g2) / B
    lc = (h * l1 + (B - h) * l2) / B
    assert abs(l - lc) / lc < 1e-4
    assert float((g - gc).norm() / gc.norm()) < 2e-3


@pytest.mark.parametrize("reduction", ["mean", "sum_over_batch"])
def test_prior_loss_under_the_ve_sde_vs_oracle(reduction):
    """DPoser prior with training.sde = 'vesde' (smplify.py:38-40 builds it; the fused prior kernel covers sub-VP / VP): the unfused path --
    HIP score function + the reference's elementwise steps -- against the oracle's VE class, loss and gradient w.r.t. the poses."""
    from dposer_amd.algorithms.advanced import sde_lib
    from dposer_amd.prior import prior_loss
    cfg, m, p = make_model(35, precision="fp32", dropout=0.0)
    rs = np.random.RandomState(13)
    B = 40
    sde = sde_lib.VESDE(sigma_min=0.01, sigma_max=50.0, N=1000)
    x0 = rs.standard_normal((B, 63)).astype(np.float32)
    z = rs.standard_normal((B, 63)).astype(np.float32)
    for t, weighted in ((0.21, True), (0.6, False)):
        xg = _dev(x0).requires_grad_(True)
        loss = prior_loss(m, sde, xg, t, weighted=weighted, reduction=reduction, batch_size=32, z=_dev(z))
        loss.backward()
        lref, gref = R.dposer_prior_loss(p, R.VE(), torch.tensor(x0), torch.full((B,), t), torch.tensor(z), weighted=weighted,
                                         reduction=reduction, batch_size=32)
        assert abs(float(loss.detach()) - float(lref)) / abs(float(lref)) < 2e-5, (t, weighted)
        assert rel_err(t2n(xg.grad), gref.numpy()) < 2e-5, (t, weighted)


def test_vp_sde_fused_paths_vs_oracle():
    """The fused sampler (both step paths), the prior loss and the DSM gradient under the VP SDE (std = sqrt(1 - e^{2 lmc}),
    g = sqrt(beta): the other branch of the SDE scalars inside the kernels) against the oracle's VP class."""
    from dposer_amd.algorithms.advanced import losses, sampling, sde_lib
    from dposer_amd.prior import prior_loss
    cfg, m, p = make_model(33, precision="fp32", dropout=0.0)
    rs = np.random.RandomState(12)
    B, N, seed = 72, 5, 99
    # sampler
    sde = sde_lib.VPSDE(0.1, 20.0, N)
    cfg.sampling.corrector = "none"
    fn = sampling.get_sampling_fn(cfg, sde, (B, 63), lambda v: v, 1e-3, device=DEV)
    z0 = rs.standard_normal((B, 63)).astype(np.float32)
    noises = [torch.tensor(PH.normal_matrix(B, 63, PH.STREAM_EM_NOISE, i, seed)) for i in range(N)]
    ref_trajs, ref_x = R.pc_sampler(p, R.VP(N=N), torch.tensor(z0), noises)
    for stride in (0, 1):
        _, x = fn(m, z=_dev(z0), seed=seed, traj_stride=stride)
        assert rel_err(t2n(x), ref_x.numpy()) < 1e-4, stride
    # prior loss + analytic gradient
    sde1000 = sde_lib.VPSDE(0.1, 20.0, 1000)
    x0 = rs.standard_normal((B, 63)).astype(np.float32)
    z = rs.standard_normal((B, 63)).astype(np.float32)
    xg = _dev(x0).requires_grad_(True)
    loss = prior_loss(m, sde1000, xg, 0.37, weighted=True, z=_dev(z))
    loss.backward()
    lref, gref = R.dposer_prior_loss(p, R.VP(), torch.tensor(x0), torch.full((B,), 0.37), torch.tensor(z), weighted=True, reduction="mean")
    assert abs(float(loss.detach()) - float(lref)) / abs(float(lref)) < 2e-4
    assert rel_err(t2n(xg.grad), gref.numpy()) < 2e-4
    # DSM loss and gradients
    t = rs.uniform(1e-3, 1.0, B).astype(np.float32)
    fg = torch.zeros(m._num_flat, device=DEV)
    l = losses.fused_dsm_grad(m, sde1000, _dev(x0), flat_grad=fg, t=_dev(t), z=_dev(z), seed=1, step=0)
    names = R.param_names()
    leaves = {n: p[n].clone().requires_grad_(True) for n in names}
    full = dict(p)
    full.update(leaves)
    ref = R.dsm_loss(full, R.VP(), torch.tensor(x0), torch.tensor(t), torch.tensor(z))
    grads = torch.autograd.grad(ref, [leaves[n] for n in names], allow_unused=True)
    assert abs(float(l) - ref.item()) / ref.item() < 5e-5
    for n, gr, off in zip(names, grads, m._offsets):
        if gr is not None:
            assert rel_err(t2n(fg[off:off + gr.numel()]), gr.reshape(-1).numpy()) < 3e-4, n


@pytest.mark.parametrize("n_blocks,E,n_poses,pose_dim,sbs,H,B", [
    (1, 512, 21, 3, True, 1024, 200), (3, 256, 21, 3, True, 1024, 200), (1, 128, 21, 3, True, 1024, 200), (2, 512, 16, 4, True, 1024, 200),
    (2, 512, 32, 4, False, 1024, 200), (2, 384, 40, 5, True, 1024, 200), (2, 512, 1, 3, True, 1024, 200), (2, 512, 50, 3, True, 1024, 200),
    (2, 512, 55, 6, True, 1024, 200),
    # hidden_dim 512 / 2048: GroupNorm(32, H) groups of 16 / 64 channels (generic epilogues), on the 128x128 (B = 200 -> 256 rows, under
    # DPOSER_SMALL_TILE_MAX=0) and the 128x32 tiling (B = 150 -> 192 rows, which 128 does not divide)
    (2, 512, 21, 3, True, 512, 200), (2, 512, 21, 3, True, 512, 150), (2, 256, 21, 6, True, 2048, 200), (1, 512, 21, 3, True, 2048, 150)])
@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
def test_other_model_configurations_vs_oracle(n_blocks, E, n_poses, pose_dim, sbs, H, B, prec, tuning_env):
    """ScoreModelFC configurations other than the shipped one (2 blocks, embed 512, D = 63, hidden 1024, scale_by_sigma): depth
    (residual-carry logic, bucket layout), embedding width, hidden width (GroupNorm group size), data dimensions that are / are
    not multiples of the 64-column padding (64, 128, 150, 200, 330, 3) and scale_by_sigma off.  Forward, sampler step and all
    gradients vs the oracle (general, pinned at the shipped shape)."""
    from dposer_amd.algorithms.advanced import losses, sampling, sde_lib
    from dposer_amd.algorithms.advanced.model import ScoreModelFC
    from dposer_amd.configs import load_config
    cfg = load_config("configs.subvp.amass_scorefc_continuous.get_config")
    cfg.model.dropout = 0.0
    cfg.model.scale_by_sigma = sbs
    D = n_poses * pose_dim
    torch.manual_seed(n_blocks + D)
    m = ScoreModelFC(cfg, n_poses=n_poses, pose_dim=pose_dim, hidden_dim=H, embed_dim=E, n_blocks=n_blocks)
    with torch.no_grad():
        for q in m.parameters():                     # default init has zero biases / unit gains in places: make every tensor matter
            q.add_(0.05 * torch.randn_like(q))
    m.precision = prec                               # (bf16x3, round 6: every depth / width / group size at the fp32 tolerances)
    m.to(DEV).eval()
    p = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    p["sigmas"] = R.sigma_table()
    assert len(m._engine().grad_buckets) == 2 + 2 * n_blocks          # layers L-1..1, front A, front B
    if H != 1024:
        # the generic-group epilogues take the 128-wide tilings only; up to 2048 samples the default policy keeps every batch on 128x32, so
        # 128x128 -- what they get above -- is forced here, and the plan says whether it was
        import score_plan as SP
        tuning_env(DPOSER_SMALL_TILE_MAX="0")
        want = SP.MID if B == 200 else SP.SMALL
        assert SP.model_plan(m, B)[:4] == ((B + 63) // 64 * 64, want, want, want), SP.model_plan(m, B)
    rs = np.random.RandomState(n_blocks)
    x = rs.standard_normal((B, D)).astype(np.float32)
    t = rs.uniform(1e-3, 1.0, B).astype(np.float32)
    z = rs.standard_normal((B, D)).astype(np.float32)
    fw = dict(n_blocks=n_blocks, scale_by_sigma=sbs)
    with torch.no_grad():
        out = m(_dev(x), _dev(t) * 999)
    ref_out = R.scorefc_forward(p, torch.tensor(x), torch.tensor(t) * 999, **fw)
    assert rel_err(t2n(out), ref_out.numpy()) < TOL_FP32
    fg = torch.zeros(m._num_flat, device=DEV)
    l = losses.fused_dsm_grad(m, sde_lib.subVPSDE(0.1, 20.0, 1000), _dev(x), flat_grad=fg, t=_dev(t), z=_dev(z), seed=1, step=0)
    names = R.param_names(n_blocks=n_blocks)
    assert names == [k for k, _ in m.named_parameters()]
    leaves = {n: p[n].clone().requires_grad_(True) for n in names}
    full = dict(p)
    full.update(leaves)
    ref = R.dsm_loss(full, R.SubVP(), torch.tensor(x), torch.tensor(t), torch.tensor(z), **fw)
    grads = torch.autograd.grad(ref, [leaves[n] for n in names], allow_unused=True)
    assert abs(float(l) - ref.item()) / ref.item() < 5e-5
    for n, gr, off in zip(names, grads, m._offsets):
        got = fg[off:off + p[n].numel()]
        if gr is None:
            assert float(got.abs().max()) == 0.0, n
        else:
            assert rel_err(t2n(got), gr.reshape(-1).numpy()) < 3e-4, n
    # three sampler steps through both step paths
    N, seed = 3, 17
    sde = sde_lib.subVPSDE(0.1, 20.0, N)
    cfg.sampling.corrector = "none"
    fn = sampling.get_sampling_fn(cfg, sde, (B, D), lambda v: v, 1e-3, device=DEV)
    noises = [torch.tensor(PH.normal_matrix(B, D, PH.STREAM_EM_NOISE, i, seed)) for i in range(N)]
    _, ref_x = R.pc_sampler(p, R.SubVP(N=N), torch.tensor(z), noises, **fw)
    for stride in (0, 1):
        _, xs = fn(m, z=_dev(z), seed=seed, traj_stride=stride)
        assert rel_err(t2n(xs), ref_x.numpy()) < 1e-4, stride
    # prior loss (shared t) and its analytic gradient, weighted and not
    from dposer_amd.prior import prior_loss
    sde1k = sde_lib.subVPSDE(0.1, 20.0, 1000)
    for tt, weighted in ((0.31, True), (0.77, False)):
        x0 = _dev(x).requires_grad_(True)
        lp = prior_loss(m, sde1k, x0, tt, weighted=weighted, z=_dev(z))
        lp.backward()
        ref_l, ref_g = R.dposer_prior_loss(p, R.SubVP(), torch.tensor(x), torch.full((B,), tt), torch.tensor(z), weighted=weighted, **fw)
        assert abs(float(lp) - ref_l.item()) / abs(ref_l.item()) < 2e-4
        assert rel_err(t2n(x0.grad), ref_g.numpy()) < 2e-4


@pytest.mark.parametrize("H", [512, 2048])
def test_inkernel_dropout_with_other_group_sizes_vs_oracle(H):
    """Training step pieces at hidden_dim 512 / 2048 with dropout drawn in-kernel: the forward epilogue hands the decisions to
    the backward epilogue in the wider aux record; loss and every gradient vs the oracle fed the same Philox masks."""
    from dposer_amd.algorithms.advanced import losses, sde_lib
    from dposer_amd.algorithms.advanced.model import ScoreModelFC
    from dposer_amd.configs import load_config
    cfg = load_config("configs.subvp.amass_scorefc_continuous.get_config")
    cfg.model.dropout = 0.25
    torch.manual_seed(H)
    m = ScoreModelFC(cfg, n_poses=21, pose_dim=3, hidden_dim=H, embed_dim=512, n_blocks=2)
    with torch.no_grad():
        for q in m.parameters():
            q.add_(0.05 * torch.randn_like(q))
    m.precision = "fp32"
    m.to(DEV).train()
    p = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    p["sigmas"] = R.sigma_table()
    B, seed, step = 320, 5, 11
    x = np.random.RandomState(1).standard_normal((B, 63)).astype(np.float32)
    fg = torch.zeros(m._num_flat, device=DEV)
    l = losses.fused_dsm_grad(m, sde_lib.subVPSDE(0.1, 20.0, 1000), _dev(x), flat_grad=fg, seed=seed, step=step)
    t = torch.tensor(PH.uniform_t(B, step, seed))
    z = torch.tensor(PH.normal_matrix(B, 63, PH.STREAM_TRAIN_Z, step, seed))
    masks = [torch.tensor(PH.dropout_keep_mask(B, H, site, step, seed, 0.25)) for site in range(5)]
    names = R.param_names()
    leaves = {n: p[n].clone().requires_grad_(True) for n in names}
    full = dict(p)
    full.update(leaves)
    ref = R.dsm_loss(full, R.SubVP(), torch.tensor(x), t, z, drop_masks=masks, drop_p=0.25)
    grads = torch.autograd.grad(ref, [leaves[n] for n in names], allow_unused=True)
    assert abs(float(l) - ref.item()) / ref.item() < 5e-5
    for n, gr, off in zip(names, grads, m._offsets):
        if gr is not None:
            assert rel_err(t2n(fg[off:off + gr.numel()]), gr.reshape(-1).numpy()) < 3e-4, n


def test_completion_sampler_inkernel_imputation_noise_matches_oracle():
    """Completion sampling with every draw made in-kernel: predictor noise (STREAM_EM_NOISE, offset = loop index) and the two
    imputation draws of sampling.py:416-420 (STREAM_IMPUTE_A before / STREAM_IMPUTE_B after the predictor, same offsets),
    against the oracle fed the numpy restatement of those Philox streams."""
    from dposer_amd.utils.misc import create_mask
    cfg, m, p = make_model(41, precision="fp32")
    N, B, seed = 6, 48, 2024
    sde, fn = _sampler(m, cfg, N, B)
    rs = np.random.RandomState(6)
    poses = torch.tensor(rs.standard_normal((B, 63)).astype(np.float32))
    torch.manual_seed(1)
    mask, obs = create_mask(poses, part="left_arm")
    z0 = rs.standard_normal((B, 63)).astype(np.float32)
    trajs, x = fn(m, observation=obs.to(DEV), mask=mask.to(DEV), z=_dev(z0), args=_Args("completion"), seed=seed)
    nz = lambda stream, i: torch.tensor(PH.normal_matrix(B, 63, stream, i, seed))
    noises = [nz(PH.STREAM_EM_NOISE, i) for i in range(N)]
    impute = [(nz(PH.STREAM_IMPUTE_A, i), nz(PH.STREAM_IMPUTE_B, i)) for i in range(N)]
    ref_trajs, ref_x = R.pc_sampler(p, R.SubVP(N=N), torch.tensor(z0), noises, observation=obs, mask=mask, impute_noises=impute)
    assert rel_err(t2n(trajs), ref_trajs.numpy()) < 1e-4
    assert rel_err(t2n(x), ref_x.numpy()) < 1e-4


@pytest.mark.parametrize("reduce_mean,lw", [(False, False), (True, True)])
def test_generic_step_path_matches_oracle(reduce_mean, lw):
    """Loss variants the fused step does not cover (sum reduction, likelihood weighting: losses.py:124-129) go through the
    generic route -- torch autograd over the HIP forward / backward, clip_grad_norm_, FusedAdam.step(), ema.update() -- and must
    follow the oracle's step just the same.  torch.rand / randn_like are pinned by a seed and re-drawn for the oracle."""
    from dposer_amd.algorithms.advanced import losses, sde_lib
    from dposer_amd.algorithms.ema import ExponentialMovingAverage
    cfg, m, p = make_model(51, precision="fp32", dropout=0.0)
    cfg.optim.warmup = 0
    names = R.param_names()
    st = R.TrainState({k: v.clone() for k, v in p.items()}, names, ema_rate=cfg.model.ema_rate)
    opt = losses.get_optimizer(cfg, m.parameters())
    ema = ExponentialMovingAverage(m.parameters(), decay=cfg.model.ema_rate)
    sde = sde_lib.subVPSDE(0.1, 20.0, 1000)
    step_fn = losses.get_step_fn(sde, True, optimize_fn=losses.optimization_manager(cfg), reduce_mean=reduce_mean, continuous=True,
                                 likelihood_weighting=lw)
    state = dict(model=m, optimizer=opt, ema=ema, step=0)
    rs = np.random.RandomState(3)
    B = 64
    for i in range(2):
        batch = rs.standard_normal((B, 63)).astype(np.float32)
        torch.manual_seed(100 + i)
        out = step_fn(state, _dev(batch))
        torch.manual_seed(100 + i)                                            # the same draws, in the reference's order (:110-111)
        t = torch.rand(B, device=DEV) * (sde.T - 1e-5) + 1e-5
        z = torch.randn_like(_dev(batch))
        ref_loss, _, _ = R.train_step(st, R.SubVP(), torch.tensor(batch), t.cpu(), z.cpu(), warmup=0, reduce_mean=reduce_mean,
                                      likelihood_weighting=lw)
        assert abs(float(out["step_loss"].detach()) - ref_loss.item()) / abs(ref_loss.item()) < 5e-5
        for (n, prm), off in zip(m.named_parameters(), m._offsets):
            assert rel_err(t2n(prm), st.p[n].numpy()) < 2e-5, (i, n)
            assert rel_err(t2n(ema.shadow_params[names.index(n)]), st.ema[n].numpy()) < 2e-5, (i, n)


def test_embed_dim_not_multiple_of_256_at_large_batch():
    """embed_dim = 384: the time-branch GEMMs must not take the 256-channel tiling at batch sizes where the GroupNorm layers do.
    Forward and gradients at 16384 samples must agree with the same model evaluated in small chunks (which the oracle checks)."""
    from dposer_amd.algorithms.advanced import losses, sde_lib
    from dposer_amd.algorithms.advanced.model import ScoreModelFC
    from dposer_amd.configs import load_config
    cfg = load_config("configs.subvp.amass_scorefc_continuous.get_config")
    cfg.model.dropout = 0.0
    torch.manual_seed(7)
    m = ScoreModelFC(cfg, n_poses=21, pose_dim=3, hidden_dim=1024, embed_dim=384, n_blocks=2)
    m.precision = "fp32"
    m.to(DEV).eval()
    B = 16384
    x = torch.randn(B, 63, device=DEV)
    t = torch.rand(B, device=DEV) * 0.999 + 1e-3
    z = torch.randn(B, 63, device=DEV)
    with torch.no_grad():
        full = m(x, t * 999)
        parts = torch.cat([m(x[i:i + 200], t[i:i + 200] * 999) for i in range(0, B, 200)])
    assert rel_err(t2n(full), t2n(parts)) < 2e-6
    sde = sde_lib.subVPSDE(0.1, 20.0, 1000)
    g_full = torch.zeros(m._num_flat, device=DEV)
    l_full = losses.fused_dsm_grad(m, sde, x, flat_grad=g_full, t=t, z=z, seed=1, step=0)
    g_sum = torch.zeros_like(g_full)
    l_sum = 0.0
    n_chunk = 0
    for i in range(0, B, 1024):                       # mean over equal chunks of a mean-reduced loss
        gi = torch.zeros_like(g_full)
        l_sum += float(losses.fused_dsm_grad(m, sde, x[i:i + 1024], flat_grad=gi, t=t[i:i + 1024], z=z[i:i + 1024], seed=1, step=0))
        g_sum += gi
        n_chunk += 1
    assert abs(float(l_full) - l_sum / n_chunk) / abs(l_sum / n_chunk) < 1e-5
    assert rel_err(t2n(g_full), t2n(g_sum / n_chunk)) < 1e-4


@pytest.mark.parametrize("continuous", [True, False])
def test_langevin_fused_vp_sde_vs_oracle(continuous):
    """Langevin + EM under the VP SDE: alpha = sde.alphas[timestep] (sampling.py:290-292) enters the step size, the score uses
    std = sqrt(1 - e^{2 lmc}) -- or, with the discrete score function (training.continuous = False, utils.py:157-160), the DDPM table's entry
    and the label t (N - 1); injected draws, oracle step by step (pinned to the reference's own outputs: goldens g5 / g26)."""
    from dposer_amd.algorithms.advanced import sampling, sde_lib
    cfg, m, p = make_model(24, precision="fp32")
    cfg.sampling.corrector = "langevin"
    cfg.training.continuous = continuous
    N, B, start = 1000, 40, 995
    sde = sde_lib.VPSDE(0.1, 20.0, N)
    assert sampling.fused_langevin_supported(sde, m, sampling.EulerMaruyamaPredictor, sampling.LangevinCorrector, False, continuous)
    fn = sampling.get_sampling_fn(cfg, sde, (B, 63), lambda v: v, 1e-3, device=DEV)
    rs = np.random.RandomState(8)
    z0 = (rs.standard_normal((B, 63)) * 0.3).astype(np.float32)
    noise = rs.standard_normal((N - start, 2, B, 63)).astype(np.float32)
    trajs, x = fn(m, z=_dev(z0), noise=_dev(noise), start_step=start, args=_Args("denoise"))
    xo, so, ts = torch.tensor(z0), R.VP(N=N, discrete=not continuous), torch.linspace(1.0, 1e-3, N)
    for k, i in enumerate(range(start, N)):
        t = torch.ones(B) * ts[i]
        xo, _ = R.langevin_step(p, so, xo, t, torch.tensor(noise[k, 0]), snr=cfg.sampling.snr)
        xo, xm = R.em_step(p, so, xo, t, torch.tensor(noise[k, 1]))
        assert rel_err(t2n(trajs[k]), xo.numpy()) < 1e-4, i
    assert rel_err(t2n(x), xm.numpy()) < 1e-4


@pytest.mark.parametrize("continuous", [True, False])
def test_langevin_fused_ve_sde_vs_oracle(continuous):
    """Langevin + EM under the VE SDE (sde_lib.py:234-292): alpha = 1 in the step size (sampling.py:293-294), the network is conditioned on
    sigma(t) -- or, with the discrete score function (training.continuous = False), on round((T - t)(N - 1)) -- and its output is the score;
    the fused two-phase corrector + the fused predictor against the oracle step by step (the oracle itself is pinned to the reference's VE
    outputs: goldens g21 / g25)."""
    from dposer_amd.algorithms.advanced import sampling, sde_lib
    cfg, m, p = make_model(26, precision="fp32")
    cfg.sampling.corrector = "langevin"
    cfg.training.continuous = continuous
    N, B, start = 1000, 40, 995
    sde = sde_lib.VESDE(sigma_min=0.01, sigma_max=50.0, N=N)
    assert sampling.fused_langevin_supported(sde, m, sampling.EulerMaruyamaPredictor, sampling.LangevinCorrector, False, continuous)
    fn = sampling.get_sampling_fn(cfg, sde, (B, 63), lambda v: v, 1e-3, device=DEV)
    rs = np.random.RandomState(10)
    z0 = (rs.standard_normal((B, 63)) * 0.5).astype(np.float32)
    noise = rs.standard_normal((N - start, 2, B, 63)).astype(np.float32)
    trajs, x = fn(m, z=_dev(z0), noise=_dev(noise), start_step=start, args=_Args("denoise"))
    xo, so, ts = torch.tensor(z0), R.VE(0.01, 50.0, N, discrete=not continuous), torch.linspace(1.0, 1e-3, N)
    for k, i in enumerate(range(start, N)):
        t = torch.ones(B) * ts[i]
        xo, _ = R.langevin_step(p, so, xo, t, torch.tensor(noise[k, 0]), snr=cfg.sampling.snr)
        xo, xm = R.em_step(p, so, xo, t, torch.tensor(noise[k, 1]))
        assert rel_err(t2n(trajs[k]), xo.numpy()) < 1e-4, i
    assert rel_err(t2n(x), xm.numpy()) < 1e-4


@pytest.mark.parametrize("embedding", ["positional", "fourier"])
def test_langevin_fused_completion_imputation_matches_generic_loop(embedding):
    """Predictor-corrector loop with imputation (task = completion, sampling.py:416-420,455-461): per outer step the draws are
    corrector x n_steps, imputation after the corrector, predictor, imputation after the predictor.  The HIP path
    (dposer_langevin_step + dposer_em_sampler_steps with observation / mask) against the generic classes run step by step on the
    HIP score function with the same draws, n_steps = 2."""
    from unittest import mock
    from dposer_amd.algorithms.advanced import sampling, sde_lib
    from dposer_amd.utils.misc import create_mask
    cfg, m, p = make_model(25, precision="fp32", embedding=embedding)
    cfg.sampling.corrector = "langevin"
    cfg.sampling.n_steps_each = 2
    N, B, nst = 1000, 32, 2
    sde = sde_lib.subVPSDE(0.1, 20.0, N)
    rs = np.random.RandomState(9)
    poses = torch.tensor((rs.standard_normal((B, 63)) * 0.5).astype(np.float32))
    torch.manual_seed(3)
    mask, obs = create_mask(poses, part="legs")
    mask, obs = mask.to(DEV), obs.to(DEV)
    z0 = _dev((rs.standard_normal((B, 63)) * 0.3).astype(np.float32))
    # completion runs all N steps in the reference; compare the first 3 outer steps (the fused loop is driven directly)
    n_run = 3
    noise = _dev(rs.standard_normal((n_run, nst + 3, B, 63)).astype(np.float32))
    ts = torch.linspace(sde.T, 1e-3, N)
    sde_short = sde_lib.subVPSDE(0.1, 20.0, N)
    # fused: drive the first n_run steps by treating them as a "range" of the N-step schedule
    x = z0.clone()
    from dposer_amd.algorithms.advanced.sampling import fused_pc_langevin_sample
    # fused_pc_langevin_sample runs [start_step, N): run the LAST n_run steps instead, with the matching timesteps in the oracle loop
    start = N - n_run
    trajs, xf, xmf = fused_pc_langevin_sample(m, sde, x, ts, snr=cfg.sampling.snr, n_steps=nst, start_step=start, observation=obs, mask=mask,
                                              noise=noise, seed=1, traj_stride=1)
    # generic loop with the same draws
    flat = [noise[i, k] for i in range(n_run) for k in range(nst + 3)]
    it = iter(flat)
    xg = z0.clone()
    tdev = ts.to(DEV)
    with torch.no_grad(), mock.patch.object(torch, "randn_like", lambda x_, **k: next(it)):
        for i in range(start, N):
            vec_t = torch.ones(B, device=DEV) * tdev[i]
            xg, _ = sampling.shared_corrector_update_fn(xg, vec_t, obs, mask, sde, m, sampling.LangevinCorrector, True, cfg.sampling.snr, nst)
            mean, std = sde.marginal_prob(obs, vec_t)
            xg = xg * (1 - mask) + (mean + torch.randn_like(xg) * std[:, None]) * mask
            xg, xm = sampling.shared_predictor_update_fn(xg, vec_t, obs, mask, sde, m, sampling.EulerMaruyamaPredictor, False, True)
            mean, std = sde.marginal_prob(obs, vec_t)
            xg = xg * (1 - mask) + (mean + torch.randn_like(xg) * std[:, None]) * mask
            assert rel_err(t2n(trajs[i - start]), t2n(xg)) < 2e-5, i
    assert rel_err(t2n(xf), t2n(xg)) < 2e-5 and rel_err(t2n(xmf), t2n(xm)) < 2e-5


def test_auxiliary_loss_step_matches_reference_golden():
    """g17 = the reference's own get_step_fn(auxiliary_loss=True) (losses.py:91-119 multi-step denoise through the network,
    :242-258 SNR-weighted v2v / j2j terms of the posed bodies), captured with oracle.fk_torch standing in for smplx.  Here the
    same step runs on the HIP path end to end: three differentiable network evaluations whose activations stay leased, the LBS
    forward / backward of BodyModel for both bodies, clip + Adam + EMA.  fp32 mode, dropout off, injected (t, z)."""
    from dposer_amd.algorithms.advanced import losses, sde_lib
    from dposer_amd.algorithms.ema import ExponentialMovingAverage
    from dposer_amd.body_model.body_model import BodyModel
    from dposer_amd.body_model.synthetic import make_synthetic_smplx_asset
    g = load("g17_aux_loss")
    cfg, m, p = make_model(int(g["seed"]), precision="fp32", dropout=0.0)
    sde = sde_lib.subVPSDE(0.1, 20.0, 1000)
    bm = BodyModel(make_synthetic_smplx_asset(seed=0)).to(DEV)
    mean, std = _dev(g["mean"]), _dev(g["std"])
    state = dict(model=m, optimizer=losses.get_optimizer(cfg, m.parameters()), ema=ExponentialMovingAverage(m.parameters(), cfg.model.ema_rate),
                 step=int(g["step"]))
    step_fn = losses.get_step_fn(sde, True, optimize_fn=losses.optimization_manager(cfg), reduce_mean=True, continuous=True,
                                 auxiliary_loss=True, denormalize=lambda x: x * std + mean, body_model=bm, rot_rep="axis",
                                 denoise_steps=int(g["denoise_steps"]))
    t = _dev(g["u"]) * (1.0 - 1e-5) + 1e-5
    out = step_fn(state, _dev(g["batch"]), t=t, z=_dev(g["z"]))
    assert set(out) == {"step_loss", "score_loss", "v2v_loss", "j2j_loss"} and state["step"] == int(g["step"]) + 1
    for k in out:
        assert abs(float(out[k]) - float(g[k])) / abs(float(g[k])) < 2e-4, (k, float(out[k]), float(g[k]))
    worst = 0.0
    for name, prm in m.named_parameters():
        ref = g[f"grad/{name}"]
        if ref.shape[0] > 1:                                   # (pre_dense_cond: no gradient)
            worst = max(worst, rel_err(probe(name, prm.grad), ref))
        assert rel_err(probe(name, prm), g[f"param/{name}"]) < 2e-5, name
    assert worst < 2e-3, worst


def test_rk_stage_combination_kernel_returns_the_bits_of_the_torch_expression():
    """dposer_rk_combine_f64 (one launch per Runge-Kutta stage on the float64 ODE state) against the left-to-right torch
    expression it replaces, zero coefficients skipped, with and without the base vector."""
    from dposer_amd.algorithms.advanced import ode_device
    rs = np.random.RandomState(0)
    n = 8192 * 64 + 8192 + 3
    y = torch.tensor(rs.standard_normal(n), device=DEV)
    ks = [torch.tensor(rs.standard_normal(n), device=DEV) for _ in range(7)]
    for coefs, base, scale in ((ode_device._A[5], y, 0.0371), (ode_device._B, y, -0.01), (ode_device._E, None, 1.0), ((1.0, 2.0, 2.0, 1.0), y, 0.5 / 6)):
        k = ks[:len(coefs)]
        got = ode_device._combine(base, k, coefs, scale)
        terms = [(kk, c) for kk, c in zip(k, coefs) if c != 0.0]
        acc = terms[0][0] * terms[0][1]
        for kk, c in terms[1:]:
            acc = acc + kk * c
        acc = acc * scale
        ref = acc if base is None else base + acc
        assert torch.equal(got, ref)


@pytest.mark.parametrize("kind,precision", [("subvp", "fp32"), ("vp", "fp32"), ("subvp", "bf16")])
def test_fused_probability_flow_rhs_against_the_expression_path(kind, precision, monkeypatch):
    """likelihood.FusedPfRhs (dposer_pf_ode_rhs_begin / _end around the network calls) against the expression-by-expression path it
    replaces (probability_flow_drift + torch.autograd on the same HIP forward / input-gradient): the drift carries the same bits,
    the Hutchinson sum differs only by summation order; then the whole likelihood and the ODE sampler with and without it."""
    from dposer_amd.algorithms.advanced import likelihood, sampling, sde_lib
    g = load("g12_likelihood_ode")
    cfg, m, p = make_model(int(g["seed"]), precision=precision)
    sde = (sde_lib.subVPSDE if kind == "subvp" else sde_lib.VPSDE)(beta_min=0.1, beta_max=20.0, N=1000)
    rs = np.random.RandomState(5)
    B, D = 1000, 63
    noise = _dev((rs.randint(0, 2, (B, D)) * 2 - 1).astype(np.float32))
    fused = likelihood.FusedPfRhs.build(sde, m, (B, D), DEV, noise)
    drift_only = likelihood.FusedPfRhs.build(sde, m, (B, D), DEV)
    assert fused is not None and drift_only is not None
    for t in (1e-4, 0.0371, 0.5, 1.0):
        state = torch.tensor(np.concatenate([rs.standard_normal(B * D), rs.standard_normal(B)]), device=DEV)
        got = fused(t, state)
        vec_t = torch.full((B,), float(t), device=DEV, dtype=torch.float32)
        with torch.enable_grad(), m.input_grad_only():
            xg = state[:B * D].reshape(B, D).float().requires_grad_(True)
            drift = likelihood.probability_flow_drift(sde, m, xg, vec_t)
            vjp, = torch.autograd.grad((drift * noise).sum(), xg)
        want_div = (vjp * noise).flatten(1).sum(dim=1).double()
        assert got.dtype == torch.float64 and got.shape == (B * D + B,)
        assert torch.equal(got[:B * D], drift.detach().reshape(-1).double()), t
        assert rel_err(t2n(got[B * D:]), t2n(want_div)) < 2e-6, t
        with torch.no_grad():
            want = likelihood.probability_flow_drift(sde, m, state[:B * D].reshape(B, D).float(), vec_t)
        assert rel_err(t2n(drift_only(t, state[:B * D])), t2n(want.reshape(-1).double())) < (1e-6 if precision == "fp32" else 2e-2), t
    del fused, drift_only
    if precision != "fp32":
        return
    data, eps = _dev(g["data"]), _dev(g["lik_Rademacher/eps"])
    z0 = _dev(g["ode/z"]) if "ode/z" in g else torch.randn(16, D, device=DEV)
    res = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("DPOSER_ODE_FUSED_RHS", flag)
        res[flag] = [likelihood.get_likelihood_fn(sde, lambda v: v, eps=1e-4, **kw)(m, data, epsilon=eps)
                     + sampling.get_ode_sampler(sde, tuple(z0.shape), lambda v: v, device=DEV, **kw)(m, z=z0.clone())
                     for kw in (dict(method="rk4", n_steps=60), dict(rtol=1e-4, atol=1e-4))]
    # fixed steps: the same step sequence, so only the summation order of the Hutchinson term separates the two;
    # adaptive steps: the step-size controller amplifies that last-bit difference to a fraction of the solver tolerance
    for (bpd1, z1, n1, nfe1, x1), (bpd0, zz0, n0, nfe0, x0), tol in zip(res["1"], res["0"], (1e-5, 2e-3)):
        assert n1 == n0 and nfe1 == nfe0
        assert rel_err(t2n(bpd1), t2n(bpd0)) < tol and rel_err(t2n(z1), t2n(zz0)) < tol and rel_err(t2n(x1), t2n(x0)) < tol


def test_fixed_step_likelihood_and_ode_sampler():
    """method='rk4' (no step-size control, no host synchronisation) through get_likelihood_fn / get_ode_sampler: converges to the
    adaptive RK45 result of the same right-hand side as the step count grows, nfe = 4 n_steps."""
    from dposer_amd.algorithms.advanced import likelihood, sampling, sde_lib
    g = load("g12_likelihood_ode")
    cfg, m, p = make_model(int(g["seed"]), precision="fp32")
    sde = sde_lib.subVPSDE(beta_min=0.1, beta_max=20.0, N=1000)
    data, eps = _dev(g["data"]), _dev(g["lik_Rademacher/eps"])
    ref_bpd, ref_z, _ = likelihood.get_likelihood_fn(sde, lambda v: v, rtol=1e-6, atol=1e-6, eps=1e-4)(m, data, epsilon=eps)
    errs = []
    for n in (50, 400):
        bpd, z, nfe = likelihood.get_likelihood_fn(sde, lambda v: v, method="rk4", n_steps=n, eps=1e-4)(m, data, epsilon=eps)
        assert nfe == 4 * n
        errs.append(rel_err(t2n(bpd), t2n(ref_bpd)))
    assert errs[1] < 1e-3 and errs[1] < errs[0]
    with pytest.raises(ValueError):
        likelihood.get_likelihood_fn(sde, lambda v: v, method="rk4")
    nfe, x = sampling.get_ode_sampler(sde, (6, 63), lambda v: v, method="euler", n_steps=64, eps=1e-3, device=DEV)(m, z=_dev(g["ode/z"]))
    assert nfe == 64 and torch.isfinite(x).all()


def test_ve_probability_flow_ode_on_the_fused_right_hand_side(monkeypatch):
    """training.sde = 'vesde' through get_likelihood_fn / get_ode_sampler (likelihood.py:40-113, sampling.py:471-542; both build the CONTINUOUS
    score function): round 6 the VE drift -- drift0 = 0, g = sigma(t) sqrt(2 ln(sigma_max / sigma_min)), the network conditioned on sigma(t),
    its output the score -- runs on dposer_pf_ode_rhs_begin / _end like VP / sub-VP.  Against the step-by-step form
    (DPOSER_ODE_FUSED_RHS=0: the reference's torch expressions + autograd around the HIP score function): one right-hand side has the drift
    bit for bit and the Hutchinson term to its 63-term summation order; the sampler (drift only) therefore takes identical adaptive steps,
    the likelihood solve (1e-7 differences in d logp / dt under an untrained, stiff VE field) may place a few steps differently and lands on
    the same bpd / latents to the solver tolerance."""
    from dposer_amd.algorithms.advanced import likelihood, sampling, sde_lib
    g = load("g12_likelihood_ode")
    cfg, m, p = make_model(int(g["seed"]), precision="fp32")
    sde = sde_lib.VESDE(sigma_min=0.01, sigma_max=50.0, N=1000)
    data, eps = _dev(g["data"]), _dev(g["lik_Rademacher/eps"])
    B, D = data.shape
    rhs = likelihood.FusedPfRhs.build(sde, m, (B, D), DEV, eps)
    assert rhs is not None
    state = torch.cat([data.reshape(-1).double(), torch.zeros(B, dtype=torch.float64, device=DEV)])
    drift_fn = lambda xx, tt: likelihood.probability_flow_drift(sde, m, xx, tt)
    for t in (0.9, 0.5, 0.1, 1e-3):
        got = rhs(t, state)
        vt = torch.full((B,), t, device=DEV)
        want_drift = drift_fn(data, vt).detach().reshape(-1).double()
        want_div = likelihood.get_div_fn(drift_fn)(data, vt, eps).double()
        assert torch.equal(got[:B * D], want_drift), t
        assert rel_err(t2n(got[B * D:]), t2n(want_div)) < 1e-6, t
    out = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("DPOSER_ODE_FUSED_RHS", flag)
        bpd, z, nfe = likelihood.get_likelihood_fn(sde, lambda v: v, rtol=1e-5, atol=1e-5, eps=1e-5)(m, data, epsilon=eps)
        nfe_s, x = sampling.get_ode_sampler(sde, (6, 63), lambda v: v, rtol=1e-5, atol=1e-5, eps=1e-3, device=DEV)(m, z=_dev(g["ode/z"]) * 50.0)
        out[flag] = (t2n(bpd), t2n(z), nfe, nfe_s, t2n(x))
    monkeypatch.delenv("DPOSER_ODE_FUSED_RHS")
    f, u = out["1"], out["0"]
    assert f[3] == u[3] and f[3] > 0 and np.array_equal(f[4], u[4])         # drift-only solve: identical step decisions, identical samples
    assert 0 < f[2] and abs(f[2] - u[2]) <= 0.1 * u[2]
    assert np.isfinite(f[0]).all() and np.isfinite(f[4]).all()
    assert rel_err(f[0], u[0]) < 1e-4 and rel_err(f[1], u[1]) < 1e-3


@pytest.mark.parametrize("act", ["elu", "relu", "lrelu"])
@pytest.mark.parametrize("prec,tol,tol_g", [("fp32", 2e-5, 2e-4), ("bf16", 1e-2, 1e-2), ("bf16x3", 2e-5, 2e-4)])      # bf16x3 (round 6): fp32 tolerances on the bf16 pipe
def test_other_activations_vs_reference_golden(act, prec, tol, tol_g, tuning_env):
    """config.model.nonlinearity = elu / relu / lrelu (model.py:54-66 get_act): forward, DSM loss and every parameter gradient of
    the fused training path against g19 (the reference itself), through the runtime-activation epilogues of the 128-wide
    tilings -- at a ragged batch (128 x 32 tiling) and, replicated 16 x under DPOSER_SMALL_TILE_MAX=0, at a batch the 128 x 128 tiling
    takes (384 samples; the default policy has it from 2048 samples up).  The mean over 16 copies of the batch is the mean over the
    batch: the replicated training step has the golden's loss and gradients."""
    import score_plan as SP
    g = load("g19_activations")
    cfg, m, p = make_model(int(g["seed"]), precision=prec, dropout=0.0, nonlinearity=act)
    batch, t = _dev(g["batch"]), _dev(g["t"])
    tt = _dev(g["u"]) * (1.0 - 1e-5) + 1e-5
    assert SP.model_plan(m, batch.shape[0])[1:4] == (SP.SMALL, SP.SMALL, SP.SMALL)
    with torch.no_grad():
        out = m(batch, t * 999)
    assert rel_err(t2n(out), g[f"{act}_model"]) < tol

    def check_step(loss, fg):
        assert abs(loss - float(g[f"{act}_loss"])) / float(g[f"{act}_loss"]) < (2e-3 if prec == "bf16" else 1e-4)
        worst = 0.0
        for (name, prm), off in zip(m.named_parameters(), m._offsets):
            ref = g[f"{act}_grad/{name}"]
            if ref.shape[0] > 1:
                worst = max(worst, rel_err(probe(name, fg[off:off + prm.numel()].reshape(prm.shape)), ref))
        # (relu / lrelu have a step derivative: a bf16-rounded pre-activation next to zero flips the gate, measured 1.2e-2)
        assert worst < (3 * tol_g if (prec == "bf16" and act != "elu") else tol_g), worst

    check_step(*_fused_grad(m, batch, tt, _dev(g["z"])))
    tuning_env(DPOSER_SMALL_TILE_MAX="0")
    n = 16 * batch.shape[0]                                              # 384 samples: 128 x 128 tiles
    assert SP.model_plan(m, n)[:4] == (384, SP.MID, SP.MID, SP.MID), SP.model_plan(m, n)
    with torch.no_grad():
        out16 = m(batch.repeat(16, 1), (t * 999).repeat(16))
    assert rel_err(t2n(out16[:24]), g[f"{act}_model"]) < tol
    assert rel_err(t2n(out16[-24:]), g[f"{act}_model"]) < tol
    check_step(*_fused_grad(m, batch.repeat(16, 1), tt.repeat(16), _dev(g["z"]).repeat(16, 1)))


def test_fused_adam_weight_decay_follows_torch():
    """config.optim.weight_decay != 0 (losses.py:35-36): torch.optim.Adam's L2 form, grad += weight_decay * param after the clip and
    before the moments -- the fused kernel against torch.optim.Adam on the same gradients, three steps."""
    from dposer_amd.algorithms.advanced import losses
    cfg, m, p = make_model(7, precision="fp32", dropout=0.0)
    cfg.optim.weight_decay = 0.05
    opt = losses.get_optimizer(cfg, m.parameters())
    ref_params = [q.detach().clone().requires_grad_(True) for q in m.parameters()]
    ref_opt = torch.optim.Adam(ref_params, lr=cfg.optim.lr, betas=(cfg.optim.beta1, 0.999), eps=cfg.optim.eps, weight_decay=0.05)
    gen = torch.Generator(device=DEV).manual_seed(3)
    for step in range(3):
        for q, r in zip(m.parameters(), ref_params):
            g = torch.randn(q.shape, device=DEV, generator=gen) * 0.01
            q.grad, r.grad = g.clone(), g.clone()
        opt.step()
        ref_opt.step()
    for (name, q), r in zip(m.named_parameters(), ref_params):
        assert (q - r).abs().max() <= 2e-6 * max(1.0, float(r.abs().max())), name


@pytest.mark.parametrize("n_blocks,n_poses,pose_dim,embedding,precision,B", [
    (2, 21, 3, "positional", "bf16", 320), (2, 21, 3, "positional", "fp32", 96), (1, 49, 3, "positional", "bf16", 200),
    (3, 21, 6, "positional", "bf16", 128)])
def test_optimizer_step_that_repacks_the_weights_keeps_every_bit(n_blocks, n_poses, pose_dim, embedding, precision, B, monkeypatch):
    """dposer_scorefc_adam_pack_step = Adam + clip + EMA and the re-packing of the weights in one pass over the optimizer state: four
    training steps (warm-up learning rates, dropout on) with an evaluation step in between (EMA copy_to / restore rewrite the
    parameters through .data: the packed copies must be rebuilt then) end in bitwise the parameters, moments, EMA shadow and packed
    bytes of the two-kernel path (dposer_adam_ema_clip_step_wd + dposer_scorefc_pack at the start of the next step,
    DPOSER_ADAM_REPACK=0).  Shapes: the shipped one, fp32 mode, one block with D = 147 (64-column padding of the first / last
    layer), three blocks with D = 126."""
    from dposer_amd.algorithms.advanced import losses, sde_lib
    from dposer_amd.algorithms.advanced.model import ScoreModelFC
    from dposer_amd.algorithms.ema import ExponentialMovingAverage
    from dposer_amd.configs import load_config
    D = n_poses * pose_dim
    rs = np.random.RandomState(D + n_blocks)
    xs = [_dev(rs.standard_normal((B, D)).astype(np.float32)) for _ in range(5)]

    def run(repack):
        monkeypatch.setenv("DPOSER_ADAM_REPACK", "1" if repack else "0")
        cfg = load_config("configs.subvp.amass_scorefc_continuous.get_config")
        cfg.model.embedding_type = embedding
        cfg.optim.warmup = 3
        torch.manual_seed(5)
        m = ScoreModelFC(cfg, n_poses=n_poses, pose_dim=pose_dim, hidden_dim=1024, embed_dim=512, n_blocks=n_blocks)
        m.precision = precision
        m.to(DEV)
        sde = sde_lib.subVPSDE(0.1, 20.0, 1000)
        opt = losses.get_optimizer(cfg, m.parameters())
        ema = ExponentialMovingAverage(m.parameters(), decay=cfg.model.ema_rate)
        state = dict(optimizer=opt, model=m, ema=ema, step=0)
        train = losses.get_step_fn(sde, train=True, optimize_fn=losses.optimization_manager(cfg), reduce_mean=True, continuous=True)
        evalf = losses.get_step_fn(sde, train=False, optimize_fn=losses.optimization_manager(cfg), reduce_mean=True, continuous=True)
        eng = m._engine()
        losses_ = []
        n_packs = []
        for i in range(4):
            g0 = eng._pack_gen
            losses_.append(float(train(state, xs[i])["step_loss"]))
            n_packs.append(eng._pack_gen - g0)
            if i == 1:
                torch.manual_seed(9)
                evalf(state, xs[4])                      # EMA copy_to / restore in between
        if not repack:
            eng.packed(m.flat_params(), with_backward=True, force=True)
        torch.cuda.synchronize()
        return (m.flat_params().clone(), opt._flat_m.clone(), opt._flat_v.clone(), ema.flat_shadow_for(m.flat_params()).clone(),
                eng._packed.clone(), losses_, n_packs)

    a, b = run(True), run(False)
    assert a[5] == b[5]
    for name, x, y in zip(("params", "exp_avg", "exp_avg_sq", "ema", "packed"), a[:5], b[:5]):
        assert torch.equal(x, y), name
    # step 0 packs once (nothing was packed yet), then the optimizer keeps the copies current: one generation bump per step, by the
    # optimizer; the step after the evaluation step has to pack again, plus the optimizer's bump
    assert a[6] == [2, 1, 2, 1], a[6]
    assert b[6] == [1, 1, 1, 1], b[6]


def test_writes_through_the_flat_buffer_invalidate_the_optimizer_packed_weights(monkeypatch):
    """The parameters are ``.data`` views of ONE flat buffer with version counters of their own: ``flat.copy_(snapshot)`` (and the
    c10d collectives that rewrite the buffer) bump only the FLAT tensor's counter / nothing at all.  After the optimizer-that-repacks
    has left its freshness key, such a write must still force a re-pack: fused step, restore a snapshot through the flat buffer, fused
    step -- bitwise the path that always re-packs (DPOSER_ADAM_REPACK=0)."""
    from dposer_amd.algorithms.advanced import losses, sde_lib
    from dposer_amd.algorithms.advanced.model import ScoreModelFC
    from dposer_amd.algorithms.ema import ExponentialMovingAverage
    from dposer_amd.configs import load_config
    from dposer_amd import distributed as ddp
    rs = np.random.RandomState(3)
    xs = [_dev(rs.standard_normal((192, 63)).astype(np.float32)) for _ in range(3)]

    def run(repack, via):
        monkeypatch.setenv("DPOSER_ADAM_REPACK", "1" if repack else "0")
        cfg = load_config("configs.subvp.amass_scorefc_continuous.get_config")
        cfg.optim.warmup = 2
        torch.manual_seed(5)
        m = ScoreModelFC(cfg, n_poses=21, pose_dim=3, hidden_dim=1024, embed_dim=512, n_blocks=2).to(DEV)
        sde = sde_lib.subVPSDE(0.1, 20.0, 1000)
        state = dict(optimizer=losses.get_optimizer(cfg, m.parameters()), model=m, ema=ExponentialMovingAverage(m.parameters(), decay=0.999), step=0)
        train = losses.get_step_fn(sde, train=True, optimize_fn=losses.optimization_manager(cfg), reduce_mean=True, continuous=True)
        snap = m.flat_params().clone()
        out = [float(train(state, xs[0])["step_loss"]), float(train(state, xs[1])["step_loss"])]
        if via == "copy":
            m.flat_params().copy_(snap)                       # bumps flat._version only
        else:
            m.flat_params().data.copy_(snap)                  # what a collective does: no counter at all ...
            ddp._bump_param_epoch()                           # ... distributed.broadcast_ / all_gather_flat_ bump the epoch instead
        out.append(float(train(state, xs[2])["step_loss"]))
        torch.cuda.synchronize()
        return out, m.flat_params().clone()

    ref = run(False, "copy")
    for via in ("copy", "epoch"):
        got = run(True, via)
        assert got[0] == ref[0], (via, got[0], ref[0])
        assert torch.equal(got[1], ref[1]), via


def test_train_steps_with_the_reference_dropout_masks_match_the_reference_golden():
    """Closes the dropout chain directly: golden g4 holds the REFERENCE's own recorded training steps (steps 0, 1, 2, 4999, 5000 of
    get_step_fn with dropout 0.1) together with the keep masks torch's generator drew.  Those masks are fed through the fused HIP step
    (test hook dposer_scorefc_debug_set_dropout_masks: the training epilogue takes its keep decisions from them instead of Philox) and
    loss, learning rate, parameters, Adam moments and EMA shadows are compared with the reference's values themselves -- no oracle in
    between (round 3 went HIP == oracle without dropout, oracle == g4 with masks).  The injected-mask branch exists only in the
    test-hook build of the library (libdposer_hip_testhooks.so, -DDPOSER_TEST_HOOKS: the shipped training epilogue carries no such
    branch), which a process must load from the start: the body runs in a child process with DPOSER_LIB_PATH pointing at it."""
    import os
    if not os.environ.get("DPOSER_HOOKS_CHILD"):
        import subprocess
        import sys
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        lib = os.path.join(root, "dposer_amd", "libdposer_hip_testhooks.so")
        assert os.path.exists(lib), "build the test-hook library: make -C dposer_amd/csrc (target ../libdposer_hip_testhooks.so)"
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_gpu_score.py"), "-m", "gpu", "-q", "-x", "-k",
                            "test_train_steps_with_the_reference_dropout_masks_match_the_reference_golden"],
                           cwd=root, env=dict(os.environ, DPOSER_HOOKS_CHILD="1", DPOSER_LIB_PATH=lib), capture_output=True, text=True, timeout=900)
        assert r.returncode == 0 and "1 passed" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
        return
    from dposer_amd import _C
    from dposer_amd.algorithms.advanced import losses, sde_lib
    from dposer_amd.algorithms.ema import ExponentialMovingAverage
    assert _C.LIB_PATH.endswith("libdposer_hip_testhooks.so")
    g = load("g4_train_steps")
    cfg, m, p = make_model(int(g["seed"]), precision="fp32", dropout=0.1)
    sde = sde_lib.subVPSDE(0.1, 20.0, 1000)
    opt = losses.get_optimizer(cfg, m.parameters())
    ema = ExponentialMovingAverage(m.parameters(), decay=cfg.model.ema_rate)
    state = dict(optimizer=opt, model=m, ema=ema, step=0)
    step_fn = losses.get_step_fn(sde, train=True, optimize_fn=losses.optimization_manager(cfg), reduce_mean=True, continuous=True)
    names = R.param_names()
    batch = g["batch"]
    B = batch.shape[0]
    eng = m._engine()
    try:
        for i in range(5):
            s = int(g[f"s{i}_step"])
            state["step"] = s
            keep = torch.tensor(np.ascontiguousarray(g[f"s{i}_keep"]), dtype=torch.uint8, device=DEV)          # [5 sites, B, 1024]
            assert keep.shape == (5, B, 1024) and 0.85 < float(keep.float().mean()) < 0.95
            _C.check(eng.lib.dposer_scorefc_debug_set_dropout_masks(eng.h, _C.ptr(keep), B), "set_dropout_masks")
            t = torch.tensor(g[f"s{i}_u"]) * (1.0 - 1e-5) + 1e-5
            z = torch.tensor(g[f"s{i}_z"])
            out = step_fn(state, _dev(batch), t=t.to(DEV), z=z.to(DEV))
            torch.cuda.synchronize()
            assert abs(float(out["step_loss"]) - float(g[f"s{i}_loss"])) / float(g[f"s{i}_loss"]) < 5e-5, i
            assert abs(opt.param_groups[0]["lr"] - float(g[f"s{i}_lr"])) < 1e-12
            for n, prm in m.named_parameters():                # (the golden holds norm + probe entries of every tensor: helpers.probe)
                assert rel_err(probe(n, prm), g[f"s{i}_param/{n}"]) < 2e-5, (i, n)
                assert rel_err(probe(n, ema.shadow_params[names.index(n)]), g[f"s{i}_ema/{n}"]) < 2e-5, (i, n)
                if f"s{i}_m/{n}" in g.files:
                    assert rel_err(probe(n, opt.state[prm]["exp_avg"]), g[f"s{i}_m/{n}"]) < 1e-4, (i, n)      # (measured: 4.7e-5 is the
                    assert rel_err(probe(n, opt.state[prm]["exp_avg_sq"]), g[f"s{i}_v/{n}"]) < 1e-4, (i, n)   #  largest of all 700 comparisons)
    finally:
        eng.lib.dposer_scorefc_debug_set_dropout_masks(eng.h, None, 0)


# ------------------------------------------------------------------------------------------------
# TimeMLPs (reference model.py:69-90): the secondary score model on the same GEMM family
# ------------------------------------------------------------------------------------------------
_MLP_CASES = [("swish1024", 63, 1024, 2, "swish", 31), ("lrelu64", 126, 64, 2, "lrelu", 32), ("elu256", 63, 256, 1, "elu", 33)]


def _make_mlp(D, H, nb, act, seed, prec, dropout=0.0):
    from weights import make_mlp_weights
    from dposer_amd.algorithms.advanced.model import TimeMLPs
    from dposer_amd.configs import load_config
    cfg = load_config("configs.subvp.amass_scorefc_continuous.get_config")
    cfg.model.nonlinearity = act
    cfg.model.dropout = dropout
    m = TimeMLPs(cfg, n_poses=21, pose_dim=D // 21, hidden_dim=H, n_blocks=nb)
    m.load_state_dict(make_mlp_weights(seed, D, H, nb))
    if prec is not None:
        m.precision = prec
    return m.to(DEV)


@pytest.mark.parametrize("prec,tol", [("fp32", TOL_FP32), ("bf16", TOL_BF16), ("bf16x3", TOL_FP32)])      # bf16x3: the fp32 tolerances on the bf16 matrix pipe
@pytest.mark.parametrize("tag,D,H,nb,act,seed", _MLP_CASES)
def test_timemlps_forward_and_gradients_match_reference_golden(tag, D, H, nb, act, seed, prec, tol):
    """Eval forward, gradients of a linear functional w.r.t. every parameter and the input, and the sub-VP DSM loss + gradients through
    the library's loss function (train mode, dropout 0), against what the reference's TimeMLPs produced (g22, gen_golden.py)."""
    from dposer_amd.algorithms.advanced import losses, sde_lib
    g = load("g22_timemlps")
    m = _make_mlp(D, H, nb, act, seed, prec)
    m.eval()
    x = _dev(g[f"{tag}/x"]).requires_grad_(True)
    t, c = _dev(g[f"{tag}/t"]), _dev(g[f"{tag}/c"])
    with torch.no_grad():
        assert rel_err(t2n(m(x.detach(), t)), g[f"{tag}/y"]) < tol           # inference instantiation (nothing kept)
    y = m(x, t)
    assert rel_err(t2n(y), g[f"{tag}/y"]) < tol
    (y * c).sum().backward()
    assert rel_err(t2n(x.grad), g[f"{tag}/dx"]) < 2 * tol
    for n, p in m.named_parameters():
        assert rel_err(probe(n, p.grad), g[f"{tag}/grad/{n}"]) < 3 * tol, n
        p.grad = None
    sde = sde_lib.subVPSDE(beta_min=0.1, beta_max=20.0, N=1000)
    loss_fn = losses.get_sde_loss_fn(sde, train=True, reduce_mean=True, continuous=True)
    u = _dev(g[f"{tag}/dsm_u"])
    loss = loss_fn(m, _dev(g[f"{tag}/dsm_batch"]), None, None, t=u * (sde.T - 1e-5) + 1e-5, z=_dev(g[f"{tag}/dsm_z"]))
    loss.backward()
    assert abs(loss.item() - float(g[f"{tag}/dsm_loss"])) < (5 * tol) * abs(float(g[f"{tag}/dsm_loss"]))
    for n, p in m.named_parameters():
        assert rel_err(probe(n, p.grad), g[f"{tag}/dsm_grad/{n}"]) < 5 * tol, n


@pytest.mark.parametrize("B,prec,tol", [(1, "fp32", TOL_FP32), (100, "fp32", TOL_FP32), (640, "fp32", TOL_FP32), (1280, "fp32", TOL_FP32),
                                        (100, "bf16", TOL_BF16), (1280, "bf16", TOL_BF16), (20000, "bf16", TOL_BF16),
                                        (1, "bf16x3", TOL_FP32), (100, "bf16x3", TOL_FP32), (1280, "bf16x3", TOL_FP32), (20000, "bf16x3", TOL_FP32)])
def test_timemlps_train_mode_dropout_matches_philox_restatement(B, prec, tol):
    """Train mode with p = 0.1: the keep decisions of every Dropout module come from the oracle's restatement of the epilogue's Philox
    draw (site = block index); a torch fp32 restatement of model.py:74-88 with those masks gives the output, the input gradient and
    every parameter gradient.  Ragged batch sizes exercise every tiling (64-, 128- and 256-sample padding)."""
    D, H, nb = 63, 1024, 2
    m = _make_mlp(D, H, nb, "swish", 41, prec, dropout=0.1)
    m.train()
    rs = np.random.RandomState(B)
    x = _dev(rs.standard_normal((B, D))).requires_grad_(True)
    t, c = _dev(rs.random_sample(B) * 999.0), _dev(rs.standard_normal((B, D)))
    y = m(x, t)
    (y * c).sum().backward()
    seed, step = m._rng_seed, m._rng_step
    ws = [p.detach().double() for p in m.parameters()]
    xr = x.detach().double().requires_grad_(True)
    wr = [w.clone().requires_grad_(True) for w in ws]
    h = torch.nn.functional.silu(torch.cat([xr, t.double()[:, None]], 1) @ wr[0].T + wr[1])
    kept = []
    for k in range(nb):
        keep = torch.tensor(PH.dropout_keep_mask(B, H, k, step, seed, 0.1), dtype=torch.float64, device=DEV)
        kept.append(float(keep.mean()))
        h = torch.nn.functional.silu(h @ wr[2 + 2 * k].T + wr[3 + 2 * k]) * keep / 0.9
    yr = h @ wr[-2].T + wr[-1]
    (yr * c.double()).sum().backward()
    assert all(0.85 < k < 0.95 for k in kept) or B < 16
    assert rel_err(t2n(y), t2n(yr)) < tol
    assert rel_err(t2n(x.grad), t2n(xr.grad)) < 2 * tol
    for p, r in zip(m.parameters(), wr):
        assert rel_err(t2n(p.grad), t2n(r.grad)) < 3 * tol
    # a second forward draws from the next step's counters; eval mode draws nothing
    y2 = m(x.detach(), t)
    assert not torch.equal(y2, y.detach())
    m.eval()
    with torch.no_grad():
        assert torch.equal(m(x.detach(), t), m(x.detach(), t))


def test_timemlps_default_precision_keeps_the_time_label():
    """The raw label t * 999 is an input column of TimeMLPs (model.py:89-90).  Without an explicit precision the model runs in bf16x3
    (16 bits of every operand): two labels one apart near 900 give different outputs, as in the reference; in plain bf16 they are
    the same operand (spacing 4 above 512), which an explicit `precision = 'bf16'` still selects."""
    m = _make_mlp(63, 256, 1, "elu", 33, None)
    assert m.precision == "bf16x3"
    m.eval()
    x = torch.zeros(2, 63, device=DEV)
    t = torch.tensor([900.0, 901.0], device=DEV)
    with torch.no_grad():
        y = m(x, t)
        assert float((y[0] - y[1]).abs().max()) > 0
        m.precision = "bf16"
        yb = m(x, t)
        assert torch.equal(yb[0], yb[1])


def test_timemlps_trains_with_the_fused_optimizer_and_refuses_cpu():
    """run/train.py:163-176 with config.model.type = 'TimeMLPs': the model trains through get_step_fn (optimizer + EMA on the flat
    buffer) and its loss falls; a CPU input raises (no torch fallback)."""
    from dposer_amd.algorithms.advanced import losses, sde_lib
    from dposer_amd.algorithms.ema import ExponentialMovingAverage
    from dposer_amd.configs import load_config
    cfg = load_config("configs.subvp.amass_scorefc_continuous.get_config")
    m = _make_mlp(63, 1024, 2, "swish", 43, "bf16", dropout=0.1)
    with pytest.raises(Exception, match="no CPU fallback"):
        m(torch.zeros(4, 63), torch.zeros(4))
    sde = sde_lib.subVPSDE(beta_min=0.1, beta_max=20.0, N=1000)
    opt = losses.get_optimizer(cfg, m.parameters())
    ema = ExponentialMovingAverage(m.parameters(), decay=cfg.model.ema_rate)
    state = dict(optimizer=opt, model=m, ema=ema, step=0)
    step_fn = losses.get_step_fn(sde, train=True, optimize_fn=losses.optimization_manager(cfg), reduce_mean=True, continuous=True)
    torch.manual_seed(0)
    batch = torch.randn(1280, 63, device=DEV) * 0.3
    first = last = None
    for i in range(60):
        loss = step_fn(state, batch, None, None)["step_loss"]
        if i == 0:
            first = float(loss)
        last = float(loss)
    assert np.isfinite(last) and last < first


def test_roctx_ranges_are_balanced_and_change_nothing(tmp_path):
    """DPOSER_ROCTX=1: every compute entry point pushes a roctx range named after itself (libroctx64 dlopen'ed on first use) and pops it on
    every return path.  A child process with the switch on runs a forward, then pushes a range of its own: libroctx reports nesting
    level 0 for it (the library left no range open), and the results are the bits of a child without the switch.  (That the ranges
    carry the entry points' names is what `rocprofv3 --marker-trace` shows; no test reads a trace.)"""
    import subprocess
    import sys
    code = r"""
import ctypes, os, sys, hashlib
sys.path.insert(0, os.getcwd())
import torch
from gpu_common import make_model
cfg, m, p = make_model(5, precision='bf16')
x = torch.randn(64, 63, device='cuda:0', generator=torch.Generator(device='cuda:0').manual_seed(1))
t = torch.rand(64, device='cuda:0', generator=torch.Generator(device='cuda:0').manual_seed(2)) * 999
with torch.no_grad():
    y = m(x, t)
depth = -2
if os.environ.get('DPOSER_ROCTX') == '1':
    r = ctypes.CDLL('librocprofiler-sdk-roctx.so')
    r.roctxRangePushA.argtypes = [ctypes.c_char_p]
    a = r.roctxRangePushA(b'probe')            # nesting level of the new range: 0 when the library left none open
    r.roctxRangePop()
    depth = a
print('RESULT', hashlib.sha1(y.cpu().numpy().tobytes()).hexdigest(), depth)
"""
    here = os.path.dirname(os.path.abspath(__file__))
    outs = []
    for flag in ("0", "1"):
        env = dict(os.environ, DPOSER_ROCTX=flag, PYTHONPATH=os.pathsep.join([here, os.path.join(here, "golden"), os.path.dirname(here)]))
        r = subprocess.run([sys.executable, "-c", code], env=env, cwd=os.path.dirname(here), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT")][-1].split())
    assert outs[0][1] == outs[1][1]                      # same bits with and without ranges
    assert outs[1][2] == "0"                             # every pushed range was popped again


@pytest.mark.parametrize("B", [1100, 1536, 2048])
def test_the_eight_wave_128x64_tiling_carries_the_bits_of_the_128x32_tiling(B, tuning_env):
    """Round 6: between 1024 and 2048 padded samples the GroupNorm layers (forward, training forward, dgrad) of the bf16 mode run on 128 x 64
    tiles of eight waves (SHAPE_SMALL64) instead of 128 x 32 tiles of four.  Every wave still owns one 32 x 32 sub-tile and walks K in the
    same order, and the dgrad's partial sums keep one row per 32 samples: forward output, DSM loss, every parameter gradient (dropout on)
    and four sampler steps must be bit-identical with DPOSER_SMALL64=0 -- in the single-GPU form of the backward and in the bucketed one."""
    from dposer_amd.algorithms.advanced import sampling, sde_lib
    cfg, m, p = make_model(23, precision="bf16", dropout=0.1)
    gen = torch.Generator(device=DEV).manual_seed(B)
    x = torch.randn(B, 63, device=DEV, generator=gen) * 0.5
    t = torch.rand(B, device=DEV, generator=gen) * (1 - 1e-5) + 1e-5
    z = torch.randn(B, 63, device=DEV, generator=gen)
    noise = torch.randn(4, 1, B, 63, device=DEV, generator=gen)
    sde = sde_lib.subVPSDE(0.1, 20.0, 4)
    cfg.sampling.corrector = "none"
    out = {}
    for tag, env in (("128x64", None), ("128x32", "0")):
        tuning_env(DPOSER_SMALL64=env)
        m.eval()
        with torch.no_grad():
            fwd = m(x, t * 999)
            _, xs = sampling.get_sampling_fn(cfg, sde, (B, 63), lambda v: v, 1e-3, device=DEV)(m, z=z, noise=noise)
        m.train()
        loss, fg = _fused_grad(m, x, t, z, step=3)
        # the data-parallel form of the backward (weight gradients as lane launches per layer group, a HIP event per gradient bucket)
        from dposer_amd.algorithms.advanced.losses import fused_dsm_grad
        fg_b = torch.zeros(m._num_flat, device=DEV)
        loss_b = fused_dsm_grad(m, sde_lib.subVPSDE(0.1, 20.0, 1000), x, flat_grad=fg_b, t=t, z=z, seed=m._rng_seed, step=3,
                                bucket_events=m._engine().bucket_events())
        out[tag] = (fwd.clone(), xs.clone(), loss, fg.clone(), float(loss_b), fg_b.clone())
    a, b = out["128x64"], out["128x32"]
    assert torch.isfinite(a[0]).all() and torch.isfinite(a[3]).all() and float(a[3].abs().max()) > 0
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert a[2] == b[2] and torch.equal(a[3], b[3])
    assert a[4] == b[4] and torch.equal(a[5], b[5])
    assert rel_err(t2n(a[5]), t2n(a[3])) < 1e-5            # (the bucketed form adds the weight-gradient partials in another order)
