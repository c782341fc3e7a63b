"""The multi-step (DDIM) prior loss (dposer_prior_loss_multi) and the RED-Diff regulariser (dposer_prior_red_diff) on the GPU: against the
reference's own methods (golden g31) in every precision, against the CPU oracle composition (tests/prior_variants_ref.py) at ragged batch
sizes, plus the in-kernel noise, autograd, surface-method, guard-word and argument contracts.

Bounds (rel. L2; TOL = TOL_FP32 for fp32 / bf16x3, TOL_BF16 for bf16 -- the bounds of one network evaluation, gpu_common):
  x0_hat, eps_pred, RED-Diff gradient   TOL        a relative error injected into every network output reaches the final estimate / the
                                                   gradient amplified by <= 1 (measured on the float64 oracle, see the golden's generator)
  multi-step gradient 2 w (x0 - x0_hat) TOL / 0.5  ||x0 - x0_hat|| / ||x0_hat|| >= 0.5 is asserted per case (golden condition 2)
  multi-step loss (quadratic in the above)         2 x the gradient's bound
  RED-Diff scalar                        2 x TOL   only where the golden's condition 3 holds (a 1e-3 score error moves it by <= 2e-3 rel.)
"""
import ctypes as C

import numpy as np
import pytest
import torch

from gpu_common import DEV, TOL_BF16, TOL_FP32, make_model, t2n
from helpers import load, rel_err
from oracle import philox as PH
from prior_variants_ref import multi_step_prior, oracle_sde, red_diff as red_diff_ref, red_diff_scalar_amplification

pytestmark = pytest.mark.gpu
torch.set_num_threads(8)

TOL = {"fp32": TOL_FP32, "bf16x3": TOL_FP32, "bf16": TOL_BF16}
MULTI_CASES = ["subvp_t03", "subvp_t05", "vp_t03", "vp_t05", "ve_t07"]
RED_CASES = ["subvp_t01", "subvp_t03", "subvp_t05", "vp_t01", "vp_t03", "vp_t05", "ve_t03", "ve_t07"]
MULTI_ENTRIES = [("comp_w", 10, True, "mean"), ("comp_u", 10, False, "mean"), ("smplify", 5, True, "sum_over_batch"),
                 ("md", 10, False, "sum_over_batch")]
_MODELS = {}


def _precisions(case):
    return ("fp32", "bf16x3") if case.startswith("ve") else ("fp32", "bf16", "bf16x3")      # VE: its golden distances only clear the fp32 bound


def _model(seed, prec, D=63):
    key = (seed, prec, D)
    if key not in _MODELS:
        _MODELS[key] = make_model(seed, D=D, precision=prec)
    return _MODELS[key]


def _sde(kind):
    from dposer_amd.algorithms.advanced import sde_lib
    if kind == "ve":
        return sde_lib.VESDE(sigma_min=0.01, sigma_max=50.0, N=1000)
    return (sde_lib.VPSDE if kind == "vp" else sde_lib.subVPSDE)(0.1, 20.0, 1000)


def _dev(a):
    return torch.tensor(np.asarray(a, dtype=np.float32), device=DEV)


def _scalar_err(a, b):
    a = float(a.detach()) if torch.is_tensor(a) else float(a)
    return abs(a - float(b)) / abs(float(b))


@pytest.fixture
def no_unfused(monkeypatch):
    """The step-by-step compositions get their score function from get_score_fn: make it raise, so only the one-call entries can answer."""
    from dposer_amd.algorithms.advanced import utils as mutils

    def boom(*a, **k):
        raise AssertionError("the unfused composition ran: get_score_fn was asked for a score function")

    monkeypatch.setattr(mutils, "get_score_fn", boom)


@pytest.mark.parametrize("case,prec", [(c, p) for c in MULTI_CASES for p in _precisions(c)])
def test_multi_step_prior_matches_reference_golden(case, prec, no_unfused):
    from dposer_amd.prior import multi_step_prior_eval, multi_step_time_grid, prior_loss
    g = load("g31_prior_variants")
    cfg, m, p = _model(int(g["seed"]), prec)
    sde, tol = _sde(case.split("_")[0]), TOL[prec]
    t, z = float(g[f"multi_{case}_t"]), _dev(g[f"multi_{case}_z"])
    B = g["x0"].shape[0]
    for name, N, weighted, reduction in MULTI_ENTRIES:
        assert float(g[f"multi_{case}_est{N}_x0_dist"]) >= 0.5            # condition 2: what the gradient's bound divides by
        x0 = _dev(g["x0"]).requires_grad_(True)
        loss = prior_loss(m, sde, x0, t, weighted=weighted, reduction=reduction, batch_size=B, z=z, multi_denoise=N)
        loss.backward()
        e_grad, e_loss = rel_err(t2n(x0.grad), g[f"multi_{case}_{name}_grad"]), _scalar_err(loss, g[f"multi_{case}_{name}_loss"])
        print(f"{case} {prec} {name}: grad {e_grad:.2e} (< {tol / 0.5:.1e}), loss {e_loss:.2e} (< {4 * tol:.1e})")
        assert e_grad < tol / 0.5
        assert e_loss < 2 * (tol / 0.5)
    for N in (1, 5, 10):
        _, _, est = multi_step_prior_eval(m, sde, _dev(g["x0"]), multi_step_time_grid(t, N), weighted=True, inv_n=1.0, z=z)
        e = rel_err(t2n(est), g[f"multi_{case}_est{N}"])
        print(f"{case} {prec} x0_hat N={N}: {e:.2e} (< {tol:.1e})")
        assert e < tol


@pytest.mark.parametrize("case,prec", [(c, p) for c in RED_CASES for p in _precisions(c)])
def test_red_diff_matches_reference_golden(case, prec, no_unfused):
    from dposer_amd.prior import red_diff, red_diff_eval
    g = load("g31_prior_variants")
    cfg, m, p = _model(int(g["seed"]), prec)
    sde, tol = _sde(case.split("_")[0]), TOL[prec]
    t, z = float(g[f"red_{case}_t"]), _dev(g["red_z"])
    x0 = _dev(g["x0"]).requires_grad_(True)
    loss = red_diff(m, sde, x0, t, z=z)
    loss.backward()
    _, _, eps = red_diff_eval(m, sde, _dev(g["x0"]), t, z=z)
    e_grad, e_eps = rel_err(t2n(x0.grad), g[f"red_{case}_grad"]), rel_err(t2n(eps), g[f"red_{case}_eps_pred"])
    e_loss = _scalar_err(loss, g[f"red_{case}_loss"])
    print(f"{case} {prec}: grad {e_grad:.2e}, eps_pred {e_eps:.2e} (< {tol:.1e}), scalar {e_loss:.2e} (< {2 * tol:.1e}, compared: "
          f"{bool(int(g[f'red_{case}_scalar_ok']))})")
    assert e_grad < tol
    assert e_eps < tol
    if int(g[f"red_{case}_scalar_ok"]):                                  # condition 3 of the golden's generator
        assert e_loss < 2 * tol


@pytest.mark.parametrize("B,D", [(1, 63), (100, 63), (257, 63), (1, 126), (100, 126), (257, 126)])
def test_multi_step_prior_vs_oracle_at_ragged_batches(B, D, no_unfused):
    """Beyond the golden, fp32: batches ragged against the 128- and 256-row tiles (and one sample), both data dimensions, N in {1, 5, 10},
    both reductions, at t = 0.3 under the sub-VP SDE; N = 5 under VP and N = 10 under VE (at t = 0.7: at 0.3 its estimate sits within
    0.13 of x0 and the gradient's bound has no premise) as well, so every kind meets every shape."""
    from dposer_amd.prior import multi_step_prior_eval, multi_step_time_grid, prior_loss
    cfg, m, p = _model(41, "fp32", D)
    rs = np.random.RandomState(1000 + B + D)
    x0, z = rs.standard_normal((B, D)).astype(np.float32), rs.standard_normal((B, D)).astype(np.float32)
    for N, kind, t in ((1, "subvp", 0.3), (5, "subvp", 0.3), (10, "subvp", 0.3), (5, "vp", 0.3), (10, "ve", 0.7)):
        for reduction, weighted in (("mean", N != 5), ("sum_over_batch", N == 5)):
            lref, gref, eref = multi_step_prior(p, oracle_sde(kind), torch.tensor(x0), t, torch.tensor(z), N, weighted=weighted,
                                                reduction=reduction, batch_size=32)
            assert float((torch.tensor(x0) - eref).norm() / eref.norm()) >= 0.5        # the premise of the gradient's bound
            xg = _dev(x0).requires_grad_(True)
            loss = prior_loss(m, _sde(kind), xg, t, weighted=weighted, reduction=reduction, batch_size=32, z=_dev(z), multi_denoise=N)
            loss.backward()
            assert rel_err(t2n(xg.grad), gref.numpy()) < TOL_FP32 / 0.5, (N, kind, reduction)
            assert _scalar_err(loss, lref) < 2 * (TOL_FP32 / 0.5), (N, kind, reduction)
        _, _, est = multi_step_prior_eval(m, _sde(kind), _dev(x0), multi_step_time_grid(t, N), weighted=True, inv_n=1.0, z=_dev(z))
        assert rel_err(t2n(est), eref.numpy()) < TOL_FP32, (N, kind)


@pytest.mark.parametrize("B,D", [(1, 63), (257, 63), (100, 126)])
def test_red_diff_vs_oracle_at_ragged_batches(B, D, no_unfused):
    from dposer_amd.prior import red_diff_eval
    cfg, m, p = _model(41, "fp32", D)
    rs = np.random.RandomState(2000 + B + D)
    x0, z = rs.standard_normal((B, D)).astype(np.float32), rs.standard_normal((B, D)).astype(np.float32)
    for kind, t in (("subvp", 0.3), ("vp", 0.3), ("ve", 0.3)):
        lref, gref, eref = red_diff_ref(p, oracle_sde(kind), torch.tensor(x0), t, torch.tensor(z))
        loss, grad, eps = red_diff_eval(m, _sde(kind), _dev(x0), t, z=_dev(z))
        assert rel_err(t2n(eps), eref.numpy()) < TOL_FP32, kind
        assert rel_err(t2n(grad), gref.numpy()) < TOL_FP32, kind
        # the scalar against the oracle's, under the premise of its bound (a score error reaches it amplified by <= 2)
        assert red_diff_scalar_amplification(eref, torch.tensor(z), torch.tensor(x0)) <= 2.0, kind
        assert _scalar_err(loss, lref) < 2 * TOL_FP32, kind
        # the scalar IS sum(grad * x0): checks the reduction at this shape free of the cancellation between signed terms.  The blocked sum
        # (<= 4 terms per thread, a 256-lane tree, <= 1024 block partials) rounds ~ log2(n) times: ~1e-6 of sum |terms|, bound TOL_FP32
        terms = grad.double() * _dev(x0).double()
        assert abs(float(loss) - float(terms.sum())) < TOL_FP32 * float(terms.abs().sum()), kind


def test_inkernel_noise_is_the_philox_prior_stream(no_unfused):
    from dposer_amd.prior import multi_step_prior_eval, multi_step_time_grid, red_diff_eval
    cfg, m, p = _model(41, "fp32")
    B, seed, step = 100, 4242, 7
    x0 = _dev(np.random.RandomState(5).standard_normal((B, 63)))
    z = _dev(PH.normal_matrix(B, 63, PH.STREAM_PRIOR, step, seed))
    for kind in ("subvp", "ve"):
        sde, traj = _sde(kind), multi_step_time_grid(0.3, 5)
        a = multi_step_prior_eval(m, sde, x0, traj, weighted=True, inv_n=1.0 / B, seed=seed, step=step)
        b = multi_step_prior_eval(m, sde, x0, traj, weighted=True, inv_n=1.0 / B, z=z)
        a2 = multi_step_prior_eval(m, sde, x0, traj, weighted=True, inv_n=1.0 / B, seed=seed, step=step)
        c = multi_step_prior_eval(m, sde, x0, traj, weighted=True, inv_n=1.0 / B, seed=seed, step=step + 1)
        assert _scalar_err(a[0], b[0]) < 1e-6 and rel_err(t2n(a[1]), t2n(b[1])) < 1e-6 and rel_err(t2n(a[2]), t2n(b[2])) < 1e-6
        assert all(torch.equal(u, v) for u, v in zip(a, a2))            # same key: bit-identical
        assert not torch.equal(a[2], c[2])
        a = red_diff_eval(m, sde, x0, 0.3, seed=seed, step=step)
        b = red_diff_eval(m, sde, x0, 0.3, z=z)
        a2 = red_diff_eval(m, sde, x0, 0.3, seed=seed, step=step)
        assert _scalar_err(a[0], b[0]) < 1e-6
        assert rel_err(t2n(a[1]), t2n(b[1])) < 1e-6 and rel_err(t2n(a[2]), t2n(b[2])) < 1e-6
        assert all(torch.equal(u, v) for u, v in zip(a, a2))


def test_autograd_contract(no_unfused):
    from dposer_amd.prior import multi_step_prior_eval, multi_step_time_grid, prior_loss, red_diff, red_diff_eval
    cfg, m, p = _model(41, "fp32")
    sde, B = _sde("subvp"), 40
    rs = np.random.RandomState(6)
    x0, z = _dev(rs.standard_normal((B, 63))), _dev(rs.standard_normal((B, 63)))
    _, gm, _ = multi_step_prior_eval(m, sde, x0, multi_step_time_grid(0.3, 5), weighted=True, inv_n=1.0 / x0.numel(), z=z)
    _, gr, _ = red_diff_eval(m, sde, x0, 0.3, z=z)
    for fn, gref in ((lambda x: prior_loss(m, sde, x, 0.3, z=z, multi_denoise=5), gm), (lambda x: red_diff(m, sde, x, 0.3, z=z), gr)):
        m.zero_grad(set_to_none=True)
        xg = x0.clone().requires_grad_(True)
        (3.0 * fn(xg)).backward()
        assert torch.equal(xg.grad, gref * 3.0)                           # the returned gradient times the upstream scalar
        assert all(prm.grad is None for prm in m.parameters())            # the estimate / residual is detached: nothing reaches the model
        with torch.no_grad():
            out = fn(x0)
        assert not out.requires_grad and torch.equal(out, fn(x0.clone().requires_grad_(True)).detach())


def test_multi_denoise_zero_is_todays_call(no_unfused):
    from dposer_amd.prior import prior_loss
    cfg, m, p = _model(41, "fp32")
    sde = _sde("subvp")
    rs = np.random.RandomState(8)
    x0, z = _dev(rs.standard_normal((40, 63))), _dev(rs.standard_normal((40, 63)))
    for kw in (dict(z=z), dict(seed=11, step=3)):
        outs = []
        for extra in ({}, dict(multi_denoise=0), dict(multi_denoise=False)):
            xg = x0.clone().requires_grad_(True)
            loss = prior_loss(m, sde, xg, 0.4, weighted=True, **kw, **extra)
            loss.backward()
            outs.append((loss.detach(), xg.grad))
        for o in outs[1:]:
            assert torch.equal(o[0], outs[0][0]) and torch.equal(o[1], outs[0][1])


def test_surface_methods_match_reference_golden(monkeypatch, no_unfused):
    """DPoser.DPoser_loss / DPoserComp.loss / MotionDenoise.DPoser_loss with multi_denoise=True and MotionDenoise.RED_Diff against their
    g31 entries (sub-VP, t = 0.3): the step counts 5 / 10 / 10, the reductions, one noise key per call."""
    import dposer_amd.prior as prior_mod
    from dposer_amd.dataset.AMASS import Posenormalizer
    from dposer_amd.tasks.completion import DPoserComp
    from dposer_amd.tasks.motion_denoising import MotionDenoise
    g, gn = load("g31_prior_variants"), load("g10_normalizer")
    cfg, m, p = _model(int(g["seed"]), "fp32")
    stats = {k.split("/")[-1]: torch.tensor(gn[k]) for k in gn.files if k.startswith("stats/axis_normalize")}
    nz = Posenormalizer(stats, device=DEV, normalize=True, min_max=False, rot_rep="axis")
    B, case = g["x0"].shape[0], "subvp_t03"
    t, z = float(g[f"multi_{case}_t"]), _dev(g[f"multi_{case}_z"])

    class Args:
        device = DEV
        sde_N = 1000

    seen = []
    real = prior_mod.multi_step_prior_eval

    def spy(model, sde, x0, traj, **kw):
        seen.append((len(traj) - 1, kw["weighted"], kw["inv_n"], kw["step"]))
        return real(model, sde, x0, traj, **kw)

    monkeypatch.setattr(prior_mod, "multi_step_prior_eval", spy)
    dposer = prior_mod.DPoser(batch_size=B, config_path="configs.subvp.amass_scorefc_continuous.get_config", args=Args(), model=m, normalizer=nz)
    comp = DPoserComp(m, _sde("subvp"), continuous=True, batch_size=B)
    md = MotionDenoise(cfg, Args(), m, None, sde_N=1000, batch_size=B, normalizer=nz)
    calls = [(dposer, lambda x: dposer.DPoser_loss(x, t, z=z, multi_denoise=True), "smplify", (5, True, 1.0 / B)),
             (comp, lambda x: comp.loss(x, t, weighted=True, z=z, multi_denoise=True), "comp_w", (10, True, 1.0 / (B * 63))),
             (comp, lambda x: comp.loss(x, t, z=z, multi_denoise=True), "comp_u", (10, False, 1.0 / (B * 63))),
             (md, lambda x: md.DPoser_loss(x, t, z=z, multi_denoise=True), "md", (10, False, 1.0 / B))]
    for obj, fn, name, expect in calls:
        before = obj._calls
        xg = _dev(g["x0"]).requires_grad_(True)
        loss = fn(xg)
        loss.backward()
        assert obj._calls == before + 1 and seen[-1] == expect + (obj._calls,)
        assert rel_err(t2n(xg.grad), g[f"multi_{case}_{name}_grad"]) < TOL_FP32 / 0.5
        assert _scalar_err(loss, g[f"multi_{case}_{name}_loss"]) < 2 * (TOL_FP32 / 0.5)
    before = md._calls
    xg = _dev(g["x0"]).requires_grad_(True)
    loss = md.RED_Diff(xg, float(g["red_subvp_t03_t"]), z=_dev(g["red_z"]))
    loss.backward()
    assert md._calls == before + 1
    assert rel_err(t2n(xg.grad), g["red_subvp_t03_grad"]) < TOL_FP32
    assert int(g["red_subvp_t03_scalar_ok"]) and _scalar_err(loss, g["red_subvp_t03_loss"]) < 2 * TOL_FP32
    # one-step calls of the same objects are untouched by the new argument
    assert torch.equal(comp.loss(_dev(g["x0"]), t, z=z), comp.loss(_dev(g["x0"]), t, z=z, multi_denoise=False))


def test_guard_words_and_workspace_reuse(no_unfused):
    """x0_hat, grad and eps_pred sit between 64 sentinel floats at B = 257, D = 63 (one row past two 128-row tiles, 63 of 64 columns): the
    kernels write exactly their [B, D] and nothing else.  Right after the ten-row call a one-row call of another kind on the same
    engine (the same workspace buffer, laid out anew) gives its own result."""
    from dposer_amd.prior import multi_step_prior_eval, multi_step_time_grid, prior_loss, red_diff_eval
    cfg, m, p = _model(41, "fp32")
    sde, B, D, G, S = _sde("subvp"), 257, 63, 64, -12345.0
    rs = np.random.RandomState(9)
    x0n, zn = rs.standard_normal((B, D)).astype(np.float32), rs.standard_normal((B, D)).astype(np.float32)
    x0, z = _dev(x0n), _dev(zn)

    def guarded():
        buf = torch.full((G + B * D + G,), S, dtype=torch.float32, device=DEV)
        return buf, buf[G:G + B * D].view(B, D)

    def intact(buf):
        return bool((buf[:G] == S).all()) and bool((buf[G + B * D:] == S).all()) and not bool((buf[G:G + B * D] == S).any())

    traj = multi_step_time_grid(0.3, 10)
    (b_hat, v_hat), (b_grad, v_grad), (b_eps, v_eps), (b_rg, v_rg) = guarded(), guarded(), guarded(), guarded()
    ref = multi_step_prior_eval(m, sde, x0, traj, weighted=True, inv_n=1.0 / B, z=z)
    loss, _, _ = multi_step_prior_eval(m, sde, x0, traj, weighted=True, inv_n=1.0 / B, z=z, x0_hat=v_hat, grad=v_grad)
    # ... a one-row workspace leased right behind the ten-row one: RED-Diff, then the one-step prior loss
    rloss, _, _ = red_diff_eval(m, sde, x0, 0.3, z=z, eps_pred=v_eps, grad=v_rg)
    one = prior_loss(m, sde, x0, 0.3, weighted=True, z=z)
    torch.cuda.synchronize()
    assert intact(b_hat) and intact(b_grad) and intact(b_eps) and intact(b_rg)
    assert torch.equal(loss, ref[0]) and torch.equal(v_grad, ref[1]) and torch.equal(v_hat, ref[2])
    rref, gref, eref = red_diff_ref(p, oracle_sde("subvp"), torch.tensor(x0n), 0.3, torch.tensor(zn))
    assert rel_err(t2n(v_eps), eref.numpy()) < TOL_FP32 and rel_err(t2n(v_rg), gref.numpy()) < TOL_FP32
    assert red_diff_scalar_amplification(eref, torch.tensor(zn), torch.tensor(x0n)) <= 2.0 and _scalar_err(rloss, rref) < 2 * TOL_FP32
    terms = v_rg.double() * x0.double()
    assert abs(float(rloss) - float(terms.sum())) < TOL_FP32 * float(terms.abs().sum())
    from oracle import score_ref as R
    lref, _ = R.dposer_prior_loss(p, R.SubVP(), torch.tensor(x0n), torch.full((B,), 0.3), torch.tensor(zn), weighted=True)
    assert _scalar_err(one, lref) < 2e-4                                  # (the one-step loss's own bound: test_gpu_score.py)
    # and the ten-row call again behind the one-row ones
    again = multi_step_prior_eval(m, sde, x0, traj, weighted=True, inv_n=1.0 / B, z=z)
    assert all(torch.equal(u, v) for u, v in zip(again, ref))


def test_raw_entry_refuses_bad_step_counts_and_launches_nothing():
    from dposer_amd import _C
    from dposer_amd.algorithms.advanced import sde_lib
    cfg, m, p = _model(41, "fp32")
    B, S = 16, -777.0
    eng = m._engine()
    flat = m.flat_params()
    packed = eng.packed(flat, with_backward=False)
    ws = eng.workspace(B, _C.WS_SHARED_T, 64, torch.device(DEV))
    x0 = torch.zeros(B, 63, device=DEV)
    outs = [torch.full((B, 63), S, device=DEV), torch.full((B, 63), S, device=DEV), torch.full((1,), S, device=DEV)]
    desc = sde_lib.sde_desc(_sde("subvp"), True)
    ts = (C.c_float * 66)(*([0.3] * 66))
    for n in (0, 65):
        rc = eng.lib.dposer_prior_loss_multi(eng.h, _C.ptr(flat), _C.ptr(packed), _C.ptr(ws), C.byref(desc), _C.ptr(x0), None, ts, n, 1, 1.0,
                                             _C.ptr(outs[0]), _C.ptr(outs[1]), _C.ptr(outs[2]), 0, 0, _C.ptr(eng.freq(x0.device)),
                                             _C.ptr(m.sigmas), B, _C.stream_ptr())
        assert rc == -1 and b"n_steps" in eng.lib.dposer_last_error()
        with pytest.raises(_C.DPoserHipError, match="n_steps"):
            _C.check(rc, "dposer_prior_loss_multi")
    torch.cuda.synchronize()
    assert all(bool((o == S).all()) for o in outs)                        # nothing was launched
