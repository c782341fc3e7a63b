"""Multi-step (DDIM) prior loss and RED-Diff without a GPU: the CPU oracle composition (tests/prior_variants_ref.py) against the reference's
own methods (golden g31), the ctypes signatures of the two C entries against the header, and the argument checks that need no GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from helpers import load, rel_err
from oracle import score_ref as R
from prior_variants_ref import multi_step_prior, oracle_sde, red_diff
from weights import make_weights

torch.set_num_threads(8)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MULTI_CASES = ["subvp_t03", "subvp_t05", "vp_t03", "vp_t05", "ve_t07"]
RED_CASES = ["subvp_t01", "subvp_t03", "subvp_t05", "vp_t01", "vp_t03", "vp_t05", "ve_t03", "ve_t07"]
# (golden entry, N, weighted, reduction) of the four reference methods captured with multi_denoise=True
MULTI_ENTRIES = [("comp_w", 10, True, "mean"), ("comp_u", 10, False, "mean"), ("smplify", 5, True, "sum_over_batch"),
                 ("md", 10, False, "sum_over_batch")]


def _params(g):
    p = make_weights(int(g["seed"]))
    p["sigmas"] = R.sigma_table()
    return p


def _scalar_err(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


def test_golden_lists_the_cases_and_records_its_conditions():
    g = load("g31_prior_variants")
    assert list(g["multi_cases"]) == MULTI_CASES and list(g["red_cases"]) == RED_CASES
    for case in MULTI_CASES:
        tol = 2e-5 if case.startswith("ve") else 1e-2           # the loosest tolerance the case is tested at (gpu_common)
        for N in (5, 10):
            assert float(g[f"multi_{case}_est{N}_dist_one_step"]) >= 5 * tol
        for N in (1, 5, 10):
            assert float(g[f"multi_{case}_est{N}_x0_dist"]) >= 0.5
    for case in RED_CASES:
        expected = not (case.split("_")[0] in ("subvp", "vp") and case.endswith("t05"))
        assert bool(int(g[f"red_{case}_scalar_ok"])) == expected
        if expected:
            assert float(g[f"red_{case}_scalar_amplification"]) <= 2.0


@pytest.mark.parametrize("case", MULTI_CASES)
def test_oracle_multi_step_prior_matches_reference_golden(case):
    g = load("g31_prior_variants")
    p, sde = _params(g), oracle_sde(case.split("_")[0], g)
    x0, z, t = torch.tensor(g["x0"]), torch.tensor(g[f"multi_{case}_z"]), float(g[f"multi_{case}_t"])
    B = x0.shape[0]
    for name, N, weighted, reduction in MULTI_ENTRIES:
        loss, grad, est = multi_step_prior(p, sde, x0, t, z, N, weighted=weighted, reduction=reduction, batch_size=B)
        assert rel_err(est, g[f"multi_{case}_est{N}"]) < 1e-5
        assert rel_err(grad, g[f"multi_{case}_{name}_grad"]) < 1e-5
        assert _scalar_err(loss, g[f"multi_{case}_{name}_loss"]) < 1e-5
    _, _, est1 = multi_step_prior(p, sde, x0, t, z, 1)
    assert rel_err(est1, g[f"multi_{case}_est1"]) < 1e-5


@pytest.mark.parametrize("case", RED_CASES)
def test_oracle_red_diff_matches_reference_golden(case):
    g = load("g31_prior_variants")
    p, sde = _params(g), oracle_sde(case.split("_")[0], g)
    loss, grad, eps = red_diff(p, sde, torch.tensor(g["x0"]), float(g[f"red_{case}_t"]), torch.tensor(g["red_z"]))
    assert rel_err(eps, g[f"red_{case}_eps_pred"]) < 1e-5
    assert rel_err(grad, g[f"red_{case}_grad"]) < 1e-5
    assert _scalar_err(loss, g[f"red_{case}_loss"]) < 1e-5


def test_time_grid_is_the_references_linear_interpolation():
    from dposer_amd.prior import multi_step_time_grid
    from dposer_amd.utils.misc import linear_interpolation
    for t, N in ((0.3, 5), (0.5, 10), (0.7, 1), (0.123, 64)):
        vec_t = torch.ones(4) * t
        ref = linear_interpolation(vec_t, vec_t / (2 * N), N + 1)              # completion.py:113,138
        grid = multi_step_time_grid(t, N)
        assert len(grid) == N + 1
        assert np.array_equal(np.asarray(grid, dtype=np.float32), ref[:, 0].numpy())
    assert multi_step_time_grid(0.5, 2, t_end=0.1) == [0.5, float(np.float32(0.5) * np.float32(0.5) + np.float32(0.5) * np.float32(0.1)),
                                                       float(np.float32(0.1))]


def test_new_entries_ctypes_signatures_match_the_header():
    from dposer_amd import _C
    hdr = open(os.path.join(ROOT, "include", "dposer_hip.h")).read()
    ctype_of = {"dposer_scorefc_t": _C.vp, "const float*": _C.vp, "const void*": _C.vp, "void*": _C.vp, "float*": _C.vp,
                "const dposer_sde_desc*": C.POINTER(_C.SdeDesc), "int32_t": _C.i32, "int64_t": _C.i64, "uint32_t": _C.u32, "uint64_t": _C.u64,
                "float": _C.f32}
    for name in ("dposer_prior_loss_multi", "dposer_prior_red_diff"):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/dposer_hip.h"
        args = []
        for decl in m.group(1).replace("\n", " ").split(","):
            typ, arg = decl.strip().rsplit(" ", 1)
            args.append(C.POINTER(_C.f32) if arg.endswith("_host") else ctype_of[typ.strip()])
        res, sig = _C.SIGNATURES[name]
        assert res is C.c_int and sig == args, name
        fn = getattr(_C.lib(), name)
        assert fn.restype is C.c_int and list(fn.argtypes) == args
    assert _C.lib().dposer_abi_version() == 1


def test_multi_entry_refuses_a_bad_step_count_before_anything_is_queued():
    from dposer_amd import _C
    lib = _C.lib()
    h = C.c_void_p()
    d = _C.ScoreFCDesc(63, 1024, 512, 2, _C.EMB_POSITIONAL, 1, 1000, _C.PREC_FP32, 0.1)
    assert lib.dposer_scorefc_create(C.byref(d), C.byref(h)) == 0
    try:
        fake = C.c_void_p(0x1000)
        sde = _C.SdeDesc(_C.SDE_SUBVP, 1000, 0.1, 20.0, 1.0)
        ts = (C.c_float * 66)(*([0.3] * 66))
        call = lambda sde_p, traj, n: lib.dposer_prior_loss_multi(h, fake, fake, fake, sde_p, fake, None, traj, n, 1, 1.0, fake, fake, fake, 0, 0,
                                                                  fake, fake, 16, None)
        for n in (0, 65, -1):
            assert call(C.byref(sde), ts, n) == -1 and b"n_steps" in lib.dposer_last_error()
        assert call(C.byref(sde), None, 5) == -1 and b"t_traj_host" in lib.dposer_last_error()
        assert call(None, ts, 5) == -1 and b"null argument" in lib.dposer_last_error()
        bad = _C.SdeDesc(9, 1000, 0.1, 20.0, 1.0)
        assert call(C.byref(bad), ts, 5) == -1 and b"SDE kind" in lib.dposer_last_error()
        rc = lib.dposer_prior_red_diff(h, fake, fake, fake, None, fake, None, 0.3, 1.0, fake, fake, fake, 0, 0, fake, fake, 16, None)
        assert rc == -1 and b"null argument" in lib.dposer_last_error()
        rc = lib.dposer_prior_red_diff(h, fake, fake, fake, C.byref(bad), fake, None, 0.3, 1.0, fake, fake, fake, 0, 0, fake, fake, 16, None)
        assert rc == -1 and b"SDE kind" in lib.dposer_last_error()
        for kind in (_C.SDE_VE_DISCRETE, _C.SDE_VP_DISCRETE):             # the discrete score functions: refused by both entries
            disc = _C.SdeDesc(kind, 1000, 0.1, 20.0, 1.0)
            assert call(C.byref(disc), ts, 5) == -1 and b"continuous score functions only" in lib.dposer_last_error()
            rc = lib.dposer_prior_red_diff(h, fake, fake, fake, C.byref(disc), fake, None, 0.3, 1.0, fake, fake, fake, 0, 0, fake, fake, 16, None)
            assert rc == -1 and b"continuous score functions only" in lib.dposer_last_error()
    finally:
        lib.dposer_scorefc_destroy(h)


def _cpu_model():
    from dposer_amd.algorithms.advanced.model import ScoreModelFC
    from dposer_amd.configs import load_config
    cfg = load_config("configs.subvp.amass_scorefc_continuous.get_config")
    return ScoreModelFC(cfg, n_poses=21, pose_dim=3, hidden_dim=1024, embed_dim=512, n_blocks=2)


def test_python_surface_argument_checks():
    from dposer_amd import _C
    from dposer_amd.algorithms.advanced import sde_lib
    from dposer_amd.prior import MAX_MULTI_DENOISE, prior_loss, red_diff as red_diff_fn
    m, sde = _cpu_model(), sde_lib.subVPSDE(0.1, 20.0, 1000)
    x = torch.zeros(4, 63)
    assert MAX_MULTI_DENOISE == 64
    for bad in (-1, 65, 2.5, True):                                      # (True: the reference's flag means 5 or 10 steps -- the methods take it)
        with pytest.raises(ValueError, match="multi_denoise"):
            prior_loss(m, sde, x, 0.3, multi_denoise=bad)
    with pytest.raises(ValueError, match="empty batch"):
        prior_loss(m, sde, x[:0], 0.3, multi_denoise=5)
    with pytest.raises(ValueError, match="empty batch"):
        red_diff_fn(m, sde, x[:0], 0.3)
    # no CPU fallback: the fused entries refuse host tensors
    with pytest.raises(_C.DPoserHipError, match="no CPU fallback"):
        prior_loss(m, sde, x, 0.3, multi_denoise=5)
    with pytest.raises(_C.DPoserHipError, match="no CPU fallback"):
        red_diff_fn(m, sde, x, 0.3)


def test_fused_route_is_chosen_for_the_continuous_score_functions_only():
    from dposer_amd.algorithms.advanced import sde_lib
    from dposer_amd.prior import _fused_variant_desc
    m = _cpu_model()
    for sde in (sde_lib.subVPSDE(0.1, 20.0, 1000), sde_lib.VPSDE(0.1, 20.0, 1000), sde_lib.VESDE(0.01, 50.0, 1000)):
        assert _fused_variant_desc(m, sde, True) is not None
    for sde in (sde_lib.VPSDE(0.1, 20.0, 1000), sde_lib.VESDE(0.01, 50.0, 1000)):
        assert _fused_variant_desc(m, sde, False) is None               # discrete score functions: the unfused composition
    assert _fused_variant_desc(torch.nn.Linear(63, 63), sde_lib.subVPSDE(0.1, 20.0, 1000), True) is None


def test_methods_without_multi_denoise_call_prior_loss_as_before(monkeypatch):
    """multi_denoise off: the three methods hand prior_loss exactly the arguments they always did (callers that wrap or replace
    prior_loss with its earlier signature keep working); on: the step counts 5 / 10 / 10."""
    import types
    import dposer_amd.prior as prior_mod
    import dposer_amd.tasks.completion as comp_mod
    import dposer_amd.tasks.motion_denoising as md_mod
    seen = []

    def old_signature(model, sde, x0, t, *, weighted=True, reduction="mean", batch_size=None, z=None, seed=0, step=0, continuous=True):
        seen.append(None)
        return "one-step"

    def new_signature(model, sde, x0, t, *, multi_denoise=0, **kw):
        seen.append(multi_denoise)
        return "multi"

    model = types.SimpleNamespace(_rng_seed=0)
    comp = comp_mod.DPoserComp(model, None, True, batch_size=4)
    md = types.SimpleNamespace(model=model, sde=None, batch_size=4, _calls=0, continuous=True)
    dp = types.SimpleNamespace(model=model, sde=None, batch_size=4, _calls=0, continuous=True)
    calls = [(comp_mod, lambda **k: comp.loss(None, 0.3, **k), 10), (md_mod, lambda **k: md_mod.MotionDenoise.DPoser_loss(md, None, 0.3, **k), 10),
             (prior_mod, lambda **k: prior_mod.DPoser.DPoser_loss(dp, None, 0.3, **k), 5)]
    for mod, fn, n in calls:
        monkeypatch.setattr(mod, "prior_loss", old_signature)
        assert fn() == "one-step" and fn(multi_denoise=False) == "one-step"
        monkeypatch.setattr(mod, "prior_loss", new_signature)
        assert fn(multi_denoise=True) == "multi" and seen[-1] == n
    assert comp._calls == md._calls == dp._calls == 3
