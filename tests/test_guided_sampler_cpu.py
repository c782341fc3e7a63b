"""CPU checks of the MCG / DPS guided samplers' test infrastructure and Python surface.

  golden   the oracle loop (tests/guided_ref.py: score_ref.em_guided_step + score_ref.impute) reproduces golden g33 -- the reference's own
           update_fn_guide stepped by tests/golden/gen_golden_guided.py -- within 1e-4 at every kept state, the final x and x_mean
  fp32     the oracle run in float32 stays within 1e-5 of its float64 run (10x under the GPU tests' fp32 bound): the loop is well
           conditioned, free-running comparisons are meaningful
  layout   the noise slots, the golden's cases and size, the C ABI declaration, the factory's argument checks
"""
import os

import numpy as np
import pytest
import torch

import guided_ref as G
from helpers import load, rel_err
from oracle import score_ref as R
from weights import make_weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
torch.set_num_threads(8)
_RUNS = {}


def _oracle(tag, dtype):
    """One oracle run per (case, dtype), shared by the tests."""
    key = (tag, dtype)
    if key not in _RUNS:
        g = load("g33_guided_sampler")
        q = G.case_inputs(g, tag)
        p = make_weights(int(g["seed"]))
        p["sigmas"] = R.sigma_table()
        trajs, x, x_mean = G.guided_loop(p, G.oracle_sde(q["kind"], q["N"]), torch.tensor(q["x0"]).to(dtype), q["noise"], q["obs"], q["mask"],
                                         method=q["method"], grad_step=q["grad_step"], eps=q["eps"], start_step=q["start"])
        _RUNS[key] = (trajs.numpy(), x.numpy(), x_mean.numpy(), q)
    return _RUNS[key]


def test_golden_cases_and_layout():
    g = load("g33_guided_sampler")
    tags = G.golden_cases()
    assert sorted(tags) == sorted(f"{k}_{m}_N{N}_s{s}" for k in ("subvp", "vp") for m in G.METHODS for N, s in ((1000, 600), (1000, 0), (32, 0)))
    assert float(g["grad_step"]) == 0.7 and g["obs"].shape == (8, 63)
    mask = g["mask"]
    assert set(np.unique(mask)) == {0.0, 1.0} and 0 < mask.sum() < mask.size          # legs masked, the rest observed
    for tag in tags:
        q = G.case_inputs(g, tag)
        n_kept = (q["N"] - q["start"]) // q["keep"]
        assert g[f"{tag}_trajs"].shape == (n_kept, 8, 63) and q["noise"].shape == (q["N"] - q["start"], G.noise_slots(q["method"]), 8, 63)
        assert q["keep"] == (100 if q["N"] == 1000 else 4)
        for k in ("trajs", "final", "final_mean", "x0"):
            assert np.isfinite(g[f"{tag}_{k}"]).all()
        assert np.array_equal(g[f"{tag}_trajs"][-1], g[f"{tag}_final"])
    assert G.noise_slots("dps") == 1 and G.noise_slots("mcg") == 2
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "g33_guided_sampler.npz")) < 1 << 20


@pytest.mark.parametrize("tag", G.golden_cases())
def test_oracle_loop_reproduces_the_reference(tag):
    g = load("g33_guided_sampler")
    trajs, x, x_mean, q = _oracle(tag, torch.float32)
    errs = dict(final=rel_err(x, g[f"{tag}_final"]), final_mean=rel_err(x_mean, g[f"{tag}_final_mean"]),
                trajs=max(rel_err(a, b) for a, b in zip(trajs[q["keep"] - 1::q["keep"]], g[f"{tag}_trajs"])))
    print(f"{tag}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert max(errs.values()) < 1e-4


@pytest.mark.parametrize("tag", G.golden_cases())
def test_the_fp32_oracle_stays_with_its_float64_run(tag):
    t32, x32, m32, q = _oracle(tag, torch.float32)
    t64, x64, m64, _ = _oracle(tag, torch.float64)
    worst = max(rel_err(a, b) for a, b in zip(t32, t64))
    print(f"{tag}: fp32 vs float64, worst index {worst:.2e}, final {rel_err(x32, x64):.2e}, x_mean {rel_err(m32, m64):.2e}")
    assert worst < 1e-5 and rel_err(m32, m64) < 1e-5


def test_teacher_forcing_steps_from_the_given_states():
    g = load("g33_guided_sampler")
    tag = "subvp_mcg_N32_s0"
    trajs, x, x_mean, q = _oracle(tag, torch.float32)
    p = make_weights(int(g["seed"]))
    p["sigmas"] = R.sigma_table()
    states = np.concatenate([q["x0"][None], trajs[:-1]])
    forced, _, _ = G.guided_loop(p, G.oracle_sde(q["kind"], q["N"]), torch.tensor(q["x0"]), q["noise"], q["obs"], q["mask"], method=q["method"],
                                 grad_step=q["grad_step"], eps=q["eps"], forced=states)
    assert np.array_equal(forced.numpy(), trajs)
    # a sub-range from a kept state continues the run
    sub, xs, _ = G.guided_loop(p, G.oracle_sde(q["kind"], q["N"]), torch.tensor(trajs[12]), q["noise"][13:], q["obs"], q["mask"], method=q["method"],
                               grad_step=q["grad_step"], eps=q["eps"], start_step=13)
    assert np.array_equal(sub.numpy(), trajs[13:]) and np.array_equal(xs.numpy(), x)


def test_capi_declares_the_guided_sampler():
    from dposer_amd import _C
    hdr = open(os.path.join(ROOT, "include", "dposer_hip.h")).read()
    assert "int dposer_guided_sampler(" in hdr and "DPOSER_WS_GUIDED = 3" in hdr and _C.WS_GUIDED == 3
    assert "sampling.py:191-207" in hdr and "sde_lib.py:98-109" in hdr
    res, args = _C.SIGNATURES["dposer_guided_sampler"]
    steps = _C.SIGNATURES["dposer_em_sampler_steps"][1]
    assert len(args) == len(steps) + 3 and args[:16] == steps[:16] and args[19:] == steps[16:]      # project, grad_step, nonfinite_step
    assert hasattr(_C.lib(), "dposer_guided_sampler") and _C.lib().dposer_abi_version() == 1


def test_factory_argument_checks():
    from dposer_amd.algorithms.advanced import sampling, sde_lib
    sde = sde_lib.subVPSDE(0.1, 20.0, 8)
    with pytest.raises(ValueError, match="method"):
        sampling.get_guided_sampler(sde, (4, 63), lambda v: v, "ddim")
    fn = sampling.get_guided_sampler(sde, (4, 63), lambda v: v, "MCG", device="cpu")
    obs, mask = torch.zeros(4, 63), torch.ones(4, 63)
    with pytest.raises(ValueError, match="observation and a mask"):
        fn(None, obs, None)
    with pytest.raises(ValueError, match="shape"):
        fn(None, obs[:3], mask[:3])
    with pytest.raises(ValueError, match="shape"):
        fn(None, obs, mask, z=torch.zeros(4, 62))
    with pytest.raises(ValueError, match="noise"):
        fn(None, obs, mask, noise=torch.zeros(8, 1, 4, 63))                        # MCG takes two slots per index
    with pytest.raises(ValueError, match="start_step"):
        fn(None, obs, mask, start_step=9)
    assert sampling.guided_noise_slots("mcg") == 2 and sampling.guided_noise_slots("dps") == 1


class _Plain(torch.nn.Module):
    """A CPU score model that is not a ScoreModelFC: the oracle network behind the model signature."""

    def __init__(self, p):
        super().__init__()
        self.p = p

    def forward(self, x, labels, condition=None, mask=None):
        return R.scorefc_forward(self.p, x, labels)


@pytest.mark.parametrize("method", G.METHODS)
def test_the_generic_path_is_the_oracle_loop(method):
    """Any model / SDE outside the one-call path steps update_fn_guide + the imputation expression: on a CPU model that is the oracle loop."""
    from dposer_amd.algorithms.advanced import sampling, sde_lib
    g = load("g33_guided_sampler")
    q = G.case_inputs(g, f"vp_{method}_N32_s0")
    p = make_weights(int(g["seed"]))
    p["sigmas"] = R.sigma_table()
    fn = sampling.get_guided_sampler(sde_lib.VPSDE(0.1, 20.0, 32), (8, 63), lambda v: v, method, grad_step=q["grad_step"], denoise=False,
                                     eps=q["eps"], device="cpu")
    real = torch.randn_like
    trajs, x = fn(_Plain(p), torch.tensor(q["obs"]), torch.tensor(q["mask"]), z=torch.tensor(q["x0"]), noise=torch.tensor(q["noise"]))
    assert torch.randn_like is real
    want, wx, _, _ = _oracle(f"vp_{method}_N32_s0", torch.float32)
    assert trajs.shape == (32, 8, 63) and rel_err(trajs.numpy(), want) < 1e-6 and rel_err(x.numpy(), wx) < 1e-6
    t4, _ = fn(_Plain(p), torch.tensor(q["obs"]), torch.tensor(q["mask"]), z=torch.tensor(q["x0"]), noise=torch.tensor(q["noise"]), traj_stride=4)
    assert torch.equal(t4, trajs[3::4])
