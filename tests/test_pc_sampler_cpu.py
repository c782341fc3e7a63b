"""The one-call predictor-corrector sampler without a GPU:

  loop       tests/pc_ref.py's loop on the CPU oracle reproduces every case of golden g32 (the reference's own Predictor / Corrector
             objects) to 1e-5 rel-L2 in fp32 torch -- this pins the reference the GPU tests compare against
  band       torch-fp32 evaluations of the repository's generic ReverseDiffusionPredictor / AncestralSamplingPredictor /
             AnnealedLangevinDynamics over a constant score lie inside the float64 band of pc_ref's stages on the whole time grids
  mutations  four seeded faults each push at least one element outside the band
  index      the library's host index helper (sde_dev.h, a stand-alone host program) equals (t * (N - 1) / T).long()
  routing    fused_pc_supported's table, the PF + corrector and DP + Langevin refusals included
  layout     _C.PcDesc against the header as the C compiler lays it out
"""
import ctypes as C
import os
import shutil
import subprocess
from unittest import mock

import numpy as np
import pytest
import torch

import pc_ref as P
from pc_ref import case_inputs, golden_cases as _cases, parse_tag
import sde_ref as S
from helpers import _log_measured, load, rel_err
from oracle import score_ref as R
from weights import make_weights

torch.set_num_threads(8)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
def _oracle_sde(kind, N, g):
    if kind == "ve":
        return R.VE(float(g["sigma_min"]), float(g["sigma_max"]), N=N)
    return (R.VP if kind == "vp" else R.SubVP)(N=N)


def oracle_run(g, tag, p, dtype=torch.float32):
    c, q = parse_tag(tag), case_inputs(g, tag)
    rs = np.random.RandomState(int(g["noise_seed"]))
    count = [0]

    def draw():
        count[0] += 1
        return rs.standard_normal((q["B"], 63)).astype(np.float32)

    sde = _oracle_sde(c["kind"], q["N"], g)
    table = g[f"ve_discrete_sigmas_{q['N']}"] if c["kind"] == "ve" else None
    obs = torch.tensor(g[f"{tag}_obs"]).to(dtype) if c["completion"] else None
    mask = torch.tensor(g[f"{tag}_mask"]).to(dtype) if c["completion"] else None
    trajs, x, x_mean, noise = P.pc_loop(p, sde, torch.tensor(q["z0"]).to(dtype), draw, predictor=c["predictor"], corrector=c["corrector"],
                                        n_steps_each=q["n_each"], snr=float(g["snr"]), probability_flow=c["pf"], eps=q["eps"],
                                        start_step=q["start"], observation=obs, mask=mask, table=table)
    assert count[0] == q["n_draws"], (tag, count[0], q["n_draws"])         # a draw exactly where the reference calls torch.randn_like
    return trajs, x, x_mean, noise, q


def test_fixture_covers_what_the_issue_lists_and_holds_the_tables():
    from dposer_amd.algorithms.advanced import sde_lib
    g = load("g32_pc_variants")
    tags = _cases()
    got = {(parse_tag(t)["predictor"], parse_tag(t)["corrector"]) for t in tags}
    for pred in ("reverse_diffusion", "ancestral_sampling", "none"):
        assert (pred, "none") in got and (pred, "ald") in got
    assert ("euler_maruyama", "ald") in got and ("reverse_diffusion", "langevin") in got
    assert any(parse_tag(t)["pf"] for t in tags) and any(parse_tag(t)["completion"] for t in tags)
    assert any(case_inputs(g, t)["start"] == 5 for t in tags) and sum(case_inputs(g, t)["N"] == 1000 for t in tags) == 2
    assert any(case_inputs(g, t)["n_each"] == 2 for t in tags)
    for N in (32, 1000):                                                    # the repository's SDE objects build the reference's tables, bit for bit
        assert sde_lib.VESDE(0.01, 50.0, N).discrete_sigmas.numpy().tobytes() == g[f"ve_discrete_sigmas_{N}"].tobytes()
        assert sde_lib.VPSDE(0.1, 20.0, N).discrete_betas.numpy().tobytes() == g[f"vp_discrete_betas_{N}"].tobytes()
        assert sde_lib.subVPSDE(0.1, 20.0, N).discrete_betas.numpy().tobytes() == g[f"vp_discrete_betas_{N}"].tobytes()
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "g32_pc_variants.npz")) < os.path.getsize(
        os.path.join(ROOT, "tests", "golden", "g4_train_steps.npz"))


@pytest.mark.parametrize("tag", _cases())
def test_oracle_loop_reproduces_the_reference(tag):
    g = load("g32_pc_variants")
    p = make_weights(int(g["seed"]))
    p["sigmas"] = R.sigma_table()
    trajs, x, x_mean, _, q = oracle_run(g, tag, p)
    e_final = rel_err(x_mean, g[f"{tag}_final"])                            # denoise = True: pc_sampler returns x_mean
    print(f"{tag}: final rel-L2 {e_final:.2e}")
    assert e_final < 1e-5
    if f"{tag}_trajs" in g.files:
        e_traj = rel_err(trajs[q["keep"] - 1::q["keep"]], g[f"{tag}_trajs"])
        print(f"{tag}: trajectory rel-L2 {e_traj:.2e}")
        assert e_traj < 1e-5


# ---- the band of the stages -------------------------------------------------------------------------------------------------------------
def _times(N=1000, every=1):
    """The grid of tests/test_gpu_sde_sweep.py, restated: linspace(T, 1e-3, 1000), linspace(T, 1e-5, 1000), the fp32 neighbours of the
    index boundaries of t * 999 and t * (N - 1), the exact halves of (T - t)(N - 1), and t = T, 1e-5, 1e-3."""
    grids = np.concatenate([torch.linspace(1.0, 1e-3, 1000).numpy()[::every], torch.linspace(1.0, 1e-5, 1000).numpy()[::every]])
    edge = [S.boundary_times(999), S.boundary_times(N - 1), S.half_times(N), np.asarray([1.0, 1e-5, 1e-3], np.float32)]
    return np.unique(np.concatenate([grids] + edge).astype(np.float32))


def _sde(kind, N):
    from dposer_amd.algorithms.advanced import sde_lib
    if kind == "ve":
        return sde_lib.VESDE(sigma_min=0.01, sigma_max=50.0, N=N)
    return (sde_lib.subVPSDE if kind == "subvp" else sde_lib.VPSDE)(0.1, 20.0, N)


def _table(sde):
    return (sde.discrete_sigmas if hasattr(sde, "discrete_sigmas") else sde.discrete_betas).numpy()


def _col(tb):
    return {k: (v[..., None] if isinstance(v, S.E) else v) for k, v in tb.items()}


def _const_score(sde, kind, c):
    ct = torch.tensor(c)

    def score_fn(x, t, condition=None, mask=None):
        if kind == "ve":
            return ct[None, :].expand_as(x)
        return -ct[None, :] / sde.marginal_prob(torch.zeros_like(x), t)[1][:, None]                     # utils.py:155, 162

    return score_fn


def _setup(kind, N=1000, D=63):
    rs = np.random.RandomState(12)
    t32 = _times(N)
    G = len(t32)
    c = (rs.choice([-1.0, 1.0], D) * np.exp(rs.uniform(np.log(1e-2), np.log(4.0), D))).astype(np.float32)
    x = rs.standard_normal((G, D)).astype(np.float32) * (50.0 if kind == "ve" else 1.0)
    z = rs.standard_normal((G, D)).astype(np.float32)
    sde = _sde(kind, N)
    s = S._col(S.scalars(kind, t32, N=N), 1)
    score = S._score(kind, S.E(c[None, :]), s["sd_score"])
    return sde, t32, c, x, z, s, score


def _torch_step(kind, what, pf=False, N=1000):
    """(got x_mean, got x, kwargs of the reference stage) of the repository's generic class in fp32 torch, every grid time a row."""
    from dposer_amd.algorithms.advanced import sampling
    sde, t32, c, x, z, s, score = _setup(kind, N)
    fn = _const_score(sde, kind, c)
    with mock.patch.object(torch, "randn_like", lambda a: torch.tensor(z)), torch.no_grad():
        if what == "ald":
            xo, xm = sampling.AnnealedLangevinDynamics(sde, fn, 0.16, 1).update_fn(torch.tensor(x), torch.tensor(t32), None, None)
        else:
            cls = sampling.ReverseDiffusionPredictor if what == "reverse_diffusion" else sampling.AncestralSamplingPredictor
            xo, xm = cls(sde, fn, pf).update_fn(torch.tensor(x), torch.tensor(t32))
    return xm.numpy(), xo.numpy(), dict(sde=sde, t32=t32, x=x, z=z, s=s, score=score, N=N)


def _ref(kind, what, k, pf=False, adj_shift=0, **faults):
    tb = _col(P.table_entries(kind, k["t32"], k["N"], _table(k["sde"]), adj_shift=adj_shift))
    if what == "ald":
        return P.ald_stage(kind, k["s"], tb, k["score"], k["x"], k["z"], 0.16, **faults)
    return P.predictor_stage(what, kind, k["s"], tb, k["score"], k["x"], k["z"], k["N"], pf=pf, **faults)


def _worst(name, got, ref):
    w = S.worst(got, ref)
    _log_measured("band_ratio_" + name, w)
    print(f"{name}: worst band ratio {w:.3f}")
    return w


STAGES = [(k, w, pf) for k in ("subvp", "vp", "ve") for w, pf in (("reverse_diffusion", False), ("reverse_diffusion", True), ("ald", False))] + \
         [(k, "ancestral_sampling", False) for k in ("vp", "ve")]


@pytest.mark.parametrize("kind,what,pf", STAGES, ids=[f"{k}-{w}{'-pf' if pf else ''}" for k, w, pf in STAGES])
def test_generic_classes_lie_inside_the_band(kind, what, pf):
    xm, xo, k = _torch_step(kind, what, pf)
    ref = _ref(kind, what, k, pf)
    assert np.isfinite(ref["x"].v).all() and np.isfinite(ref["x"].e).all() and np.isfinite(xo).all()
    assert _worst(f"cpu_{what}_{kind}{'_pf' if pf else ''}_x_mean", xm, ref["x_mean"]) <= 1.0
    assert _worst(f"cpu_{what}_{kind}{'_pf' if pf else ''}_x", xo, ref["x"]) <= 1.0


def test_ve_timestep_zero_is_exact():
    """timestep 0: adjacent sigma 0, the ancestral std exactly 0 with zero bound -- x == x_mean in the reference and in the float64 value."""
    xm, xo, k = _torch_step("ve", "ancestral_sampling")
    tb = P.table_entries("ve", k["t32"], k["N"], _table(k["sde"]))
    k0 = tb["k"] == 0
    assert k0.any() and (tb["adj"].v[k0] == 0).all()
    ref = _ref("ve", "ancestral_sampling", k)
    assert np.array_equal(xm[k0], xo[k0])
    assert np.array_equal(ref["x"].v[k0], ref["x_mean"].v[k0])
    # the bound of x there is x_mean's plus the rounding of the one addition `x_mean + 0 * z`: the std contributes nothing
    assert np.array_equal(ref["x"].e[k0], ref["x_mean"].e[k0] + S.U * np.abs(ref["x_mean"].v[k0]))


def test_seeded_mutations_leave_the_band():
    xm, xo, k = _torch_step("subvp", "reverse_diffusion", pf=True)
    assert _worst("mut_pf_factor_half", xm, _ref("subvp", "reverse_diffusion", k, pf=True, pf_factor=0.5)["x_mean"]) > 1.0
    xm, xo, k = _torch_step("ve", "reverse_diffusion")
    assert _worst("mut_adjacent_sigma_off_by_one", xo, _ref("ve", "reverse_diffusion", k, adj_shift=-1)["x"]) > 1.0
    xm, xo, k = _torch_step("ve", "ancestral_sampling")
    assert _worst("mut_adjacent_sigma_off_by_one_ancestral", xm, _ref("ve", "ancestral_sampling", k, adj_shift=-1)["x_mean"]) > 1.0
    for kind in ("subvp", "vp"):
        xm, xo, k = _torch_step(kind, "ald")
        assert _worst(f"mut_ald_alpha_dropped_{kind}", xm, _ref(kind, "ald", k, drop_alpha=True)["x_mean"]) > 1.0
    xm, xo, k = _torch_step("vp", "reverse_diffusion")
    assert _worst("mut_linear_sqrt_rd", xm, _ref("vp", "reverse_diffusion", k, linear_sqrt=True)["x_mean"]) > 1.0
    xm, xo, k = _torch_step("vp", "ancestral_sampling")
    assert _worst("mut_linear_sqrt_ancestral", xm, _ref("vp", "ancestral_sampling", k, linear_sqrt=True)["x_mean"]) > 1.0


# ---- the host index helper ----------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_host_index_helper_is_torchs_long(tmp_path):
    """tests/pc_index_main.hip includes sde_dev.h and prints sde_table_index for every time: equal to (t * (N - 1) / T).long() on both
    1000-point grids and the boundary times, N in {32, 1000, 2000}; pc_ref.table_index, which the band references index with, too."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "pc_index")
    cc = subprocess.run([hipcc, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "dposer_amd", "csrc"),
                         os.path.join(ROOT, "tests", "pc_index_main.hip"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stdout + cc.stderr
    for N in (32, 1000, 2000):
        ks = tuple(range(0, N, max(1, N // 40))) + (N - 1,)                 # (every k <= N - 1: boundary_times walks towards t = k / (N - 1))
        t32 = np.unique(np.concatenate([torch.linspace(1.0, 1e-3, 1000).numpy(), torch.linspace(1.0, 1e-5, 1000).numpy(),
                                        S.boundary_times(N - 1, ks=ks), np.asarray([1.0, 1e-5, 1e-3], np.float32)]).astype(np.float32))
        path = tmp_path / f"t{N}.bin"
        t32.astype(np.float32).tofile(str(path))
        got = np.asarray(subprocess.run([exe, str(N), "1.0", str(path)], check=True, capture_output=True, text=True, timeout=60).stdout.split(), np.int64)
        want = (torch.tensor(t32) * (N - 1) / 1).long().numpy()
        assert got.shape == want.shape and np.array_equal(got, want), N
        assert np.array_equal(P.table_index(t32, N), want)
        assert want.min() == 0 and want.max() == N - 1


# ---- routing ------------------------------------------------------------------------------------------------------------------------------
def test_fused_pc_supported_routing_table(monkeypatch):
    from dposer_amd import distributed as ddp
    from dposer_amd.algorithms.advanced import sampling, sde_lib
    from dposer_amd.algorithms.advanced.model import ScoreModelFC
    from dposer_amd.configs import load_config
    cfg = load_config("configs.subvp.amass_scorefc_continuous.get_config")
    m = ScoreModelFC(cfg, n_poses=21, pose_dim=3, hidden_dim=1024, embed_dim=512, n_blocks=2)
    preds = dict(none=sampling.NonePredictor, em=sampling.EulerMaruyamaPredictor, rd=sampling.ReverseDiffusionPredictor,
                 anc=sampling.AncestralSamplingPredictor)
    corrs = dict(none=sampling.NoneCorrector, ald=sampling.AnnealedLangevinDynamics, lang=sampling.LangevinCorrector)
    ok = sampling.fused_pc_supported
    for sde, cont in ((sde_lib.subVPSDE(0.1, 20.0, 32), True), (sde_lib.VPSDE(0.1, 20.0, 32), True), (sde_lib.VPSDE(0.1, 20.0, 32), False),
                      (sde_lib.VESDE(0.01, 50.0, 32), True), (sde_lib.VESDE(0.01, 50.0, 32), False)):
        subvp = isinstance(sde, sde_lib.subVPSDE)
        for pn, pred in preds.items():
            for cn, corr in corrs.items():
                assert ok(sde, m, pred, corr, False, cont) == (not (pn == "anc" and subvp)), (type(sde).__name__, pn, cn)
                # probability flow: only with corrector 'none', never with ancestral sampling
                assert ok(sde, m, pred, corr, True, cont) == (cn == "none" and pn != "anc"), (type(sde).__name__, pn, cn)
        assert ok(sde, m, None, None, False, cont)                             # predictor-only / corrector-only samplers
    sde = sde_lib.subVPSDE(0.1, 20.0, 32)
    assert not ok(sde, torch.nn.Linear(3, 3), preds["rd"], corrs["none"], False, True)          # another model
    sde.N = 64                                                                  # N changed after construction: the table is the constructor's
    assert not ok(sde, m, preds["rd"], corrs["ald"], False, True)              # ALD reads alpha from it
    assert ok(sde, m, preds["rd"], corrs["none"], False, True)                 # sub-VP reverse diffusion reads no table
    vp64 = sde_lib.VPSDE(0.1, 20.0, 32)
    vp64.N = 64
    assert not ok(vp64, m, preds["rd"], corrs["none"], False, True) and ok(vp64, m, preds["none"], corrs["none"], False, True)
    # data parallelism: Langevin keeps the per-step path with its all-reduce, everything else takes the one call on every rank
    sde = sde_lib.VPSDE(0.1, 20.0, 32)
    monkeypatch.setattr(ddp, "dp_active", lambda: True)
    for pn, pred in preds.items():
        assert not ok(sde, m, pred, corrs["lang"], False, True)
        assert ok(sde, m, pred, corrs["ald"], False, True) and ok(sde, m, pred, corrs["none"], False, True)
    assert sampling.fused_langevin_supported(sde, m, preds["em"], corrs["lang"], False, True)


def test_pc_sampler_order_of_the_fused_paths(monkeypatch):
    """get_pc_sampler asks fused_em_supported first (unchanged), then the new path, then fused_langevin_supported."""
    from dposer_amd.algorithms.advanced import sampling, sde_lib
    order = []
    for name in ("fused_em_supported", "fused_pc_supported", "fused_langevin_supported"):
        monkeypatch.setattr(sampling, name, lambda *a, _n=name: order.append(_n) and False)
    monkeypatch.setattr(sampling, "shared_corrector_update_fn", lambda x, *a, **k: (x, x))
    monkeypatch.setattr(sampling, "shared_predictor_update_fn", lambda x, *a, **k: (x, x))
    sde = sde_lib.subVPSDE(0.1, 20.0, 4)
    fn = sampling.get_pc_sampler(sde, (2, 63), sampling.ReverseDiffusionPredictor, sampling.NoneCorrector, lambda v: v, 0.16, device="cpu")
    fn(None, z=torch.zeros(2, 63))
    assert order == ["fused_em_supported", "fused_pc_supported", "fused_langevin_supported"]


def test_constructor_errors_still_surface_from_pc_sampler():
    from dposer_amd.algorithms.advanced import sampling, sde_lib
    from dposer_amd.algorithms.advanced.model import ScoreModelFC
    from dposer_amd.configs import load_config
    cfg = load_config("configs.subvp.amass_scorefc_continuous.get_config")
    m = ScoreModelFC(cfg, n_poses=21, pose_dim=3, hidden_dim=1024, embed_dim=512, n_blocks=2)
    anc = sampling.AncestralSamplingPredictor
    fn = sampling.get_pc_sampler(sde_lib.subVPSDE(0.1, 20.0, 32), (2, 63), anc, sampling.NoneCorrector, lambda v: v, 0.16, continuous=True, device="cpu")
    with pytest.raises(NotImplementedError, match="not yet supported"):
        fn(m, z=torch.zeros(2, 63))
    fn = sampling.get_pc_sampler(sde_lib.VPSDE(0.1, 20.0, 32), (2, 63), anc, sampling.NoneCorrector, lambda v: v, 0.16, probability_flow=True,
                                 continuous=True, device="cpu")
    with pytest.raises(AssertionError, match="Probability flow not supported"):
        fn(m, z=torch.zeros(2, 63))


# ---- ABI -----------------------------------------------------------------------------------------------------------------------------------
def test_pc_desc_layout_matches_the_header(tmp_path):
    from dposer_amd import _C
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dposer_hip.h"', 'int main(void) {',
             '  printf("size size %zu\\n", sizeof(dposer_pc_desc));']
    for fname, _ in _C.PcDesc._fields_:
        lines.append(f'  printf("off {fname} %zu\\n", offsetof(dposer_pc_desc, {fname}));')
    lines.append('  printf("enum pred %d\\n", DPOSER_PC_PRED_NONE + 10 * DPOSER_PC_PRED_EULER_MARUYAMA + 100 * DPOSER_PC_PRED_REVERSE_DIFFUSION + 1000 * DPOSER_PC_PRED_ANCESTRAL);')
    lines.append('  printf("enum corr %d\\n", DPOSER_PC_CORR_NONE + 10 * DPOSER_PC_CORR_LANGEVIN + 100 * DPOSER_PC_CORR_ALD);')
    lines += ['  return 0;', '}']
    src = tmp_path / "pc_probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "pc_probe"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = {}
    for ln in subprocess.check_output([str(exe)], text=True).splitlines():
        a, b, c = ln.split()
        got[(a, b)] = int(c)
    assert got[("size", "size")] == C.sizeof(_C.PcDesc)
    for fname, _ in _C.PcDesc._fields_:
        assert got[("off", fname)] == getattr(_C.PcDesc, fname).offset, fname
    assert [f for f, _ in _C.PcDesc._fields_] == ["predictor", "corrector", "n_steps_each", "probability_flow", "snr", "inv_global_batch"]
    assert got[("enum", "pred")] == _C.PC_PRED_NONE + 10 * _C.PC_PRED_EULER_MARUYAMA + 100 * _C.PC_PRED_REVERSE_DIFFUSION + 1000 * _C.PC_PRED_ANCESTRAL
    assert got[("enum", "corr")] == _C.PC_CORR_NONE + 10 * _C.PC_CORR_LANGEVIN + 100 * _C.PC_CORR_ALD
    assert "dposer_pc_sampler" in _C.SIGNATURES and hasattr(_C.lib(), "dposer_pc_sampler")
