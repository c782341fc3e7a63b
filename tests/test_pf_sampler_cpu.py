"""Probability-flow sampler without a GPU: the PF oracle loop (tests/pf_ref.py) against the reference's own deterministic sampler (golden
g28), the interpolation task's slerp segments against utils.misc.slerp_interpolation, the C entry's ctypes signature and argument checks,
and the host routing of pc_sampler."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import load, rel_err
from oracle import score_ref as R
from pf_ref import pf_sampler
from weights import make_weights

torch.set_num_threads(8)


def _params(g):
    p = make_weights(int(g["seed"]))
    p["sigmas"] = R.sigma_table()
    return p


def _oracle_sde(kind, N, g):
    if kind == "ve":
        return R.VE(float(g["sigma_min"]), float(g["sigma_max"]), N=N)
    return (R.VP if kind == "vp" else R.SubVP)(N=N)


@pytest.mark.parametrize("kind", ["subvp", "vp", "ve"])
def test_pf_oracle_matches_reference_golden(kind):
    g = load("g28_pf_sampler")
    tag = f"{kind}8"
    trajs, x = pf_sampler(_params(g), _oracle_sde(kind, 8, g), torch.tensor(g[f"{tag}_z0"]), eps=float(g[f"{tag}_eps"]))
    assert int(g[f"{tag}_n_draws"]) == 8                         # the reference draws z at every step and multiplies it by zero
    assert rel_err(trajs, g[f"{tag}_trajs"]) < 1e-5
    assert rel_err(x, g[f"{tag}_final"]) < 1e-5
    assert np.array_equal(g[f"{tag}_trajs"][-1], g[f"{tag}_final"])      # x == x_mean: no diffusion


def test_pf_oracle_completion_and_denoise_golden():
    g = load("g28_pf_sampler")
    p = _params(g)
    noise = torch.tensor(g["comp8_noise"])                      # per step: impute-after-corrector, predictor z (unused), impute-after-predictor
    assert noise.shape[0] == 3 * 8
    imp = [(noise[3 * i], noise[3 * i + 2]) for i in range(8)]
    trajs, x = pf_sampler(p, R.SubVP(N=8), torch.tensor(g["comp8_z0"]), eps=float(g["comp8_eps"]), observation=torch.tensor(g["comp8_obs"]),
                          mask=torch.tensor(g["comp8_mask"]), impute_noises=imp)
    assert rel_err(trajs, g["comp8_trajs"]) < 1e-5
    assert rel_err(x, g["comp8_final"]) < 1e-5
    trajs, x = pf_sampler(p, R.SubVP(N=8), torch.tensor(g["den8_z0"]), eps=float(g["den8_eps"]), start_step=int(g["den8_start_step"]))
    assert trajs.shape == (5, 16, 63)
    assert rel_err(trajs, g["den8_trajs"]) < 1e-5
    assert rel_err(x, g["den8_final"]) < 1e-5


def test_pf_oracle_1000_steps_golden():
    g = load("g28_pf_sampler")
    trajs, x = pf_sampler(_params(g), R.SubVP(N=1000), torch.tensor(g["pf1000_z0"]), eps=float(g["pf1000_eps"]))
    assert float(g["pf1000_eps"]) == 1e-5
    assert rel_err(trajs[99::100], g["pf1000_trajs"]) < 1e-4
    assert rel_err(x, g["pf1000_final"]) < 1e-4


def test_slerp_segments_are_slerp_interpolation_segment_by_segment():
    from dposer_amd.tasks.interpolation import slerp_segments
    from dposer_amd.utils.misc import slerp_interpolation
    z = torch.tensor(np.random.RandomState(5).standard_normal((6, 63)).astype(np.float32))
    seg = slerp_segments(z, 60)
    assert seg.shape == (5, 60, 63)
    for s in range(5):
        assert torch.equal(seg[s], slerp_interpolation(z[s], z[s + 1], 60))
    assert torch.equal(seg[:, 0], z[:-1]) and torch.equal(seg[:, -1], z[1:])      # the ends are the anchors' latents
    assert slerp_segments(z[:1], 7).shape == (0, 7, 63)


def test_pf_sampler_ctypes_signature_and_argument_checks():
    from dposer_amd import _C
    assert _C.SIGNATURES["dposer_pf_sampler"] == _C.SIGNATURES["dposer_em_sampler"]         # same arguments as the stochastic entry
    lib = _C.lib()
    fn = lib.dposer_pf_sampler
    assert fn.restype is C.c_int and list(fn.argtypes) == list(_C.SIGNATURES["dposer_em_sampler"][1])
    h = C.c_void_p()
    d = _C.ScoreFCDesc(63, 1024, 512, 2, _C.EMB_POSITIONAL, 1, 1000, _C.PREC_BF16, 0.1)
    assert lib.dposer_scorefc_create(C.byref(d), C.byref(h)) == 0
    try:
        fake = C.c_void_p(0x1000)
        ts = (C.c_float * 8)()
        # no SDE descriptor: refused before anything is queued
        rc = fn(h, fake, fake, fake, None, fake, fake, C.cast(ts, C.c_void_p), 0, None, None, None, 0, None, 1, fake, fake, 8, None)
        assert rc != 0 and b"null argument" in lib.dposer_last_error()
        sde = _C.SdeDesc(_C.SDE_SUBVP, 8, 0.1, 20.0, 1.0)
        rc = fn(h, fake, fake, fake, C.byref(sde), fake, fake, C.cast(ts, C.c_void_p), 9, None, None, None, 0, None, 1, fake, fake, 8, None)
        assert rc != 0 and b"step range" in lib.dposer_last_error()
        rc = fn(h, fake, fake, fake, C.byref(sde), fake, fake, C.cast(ts, C.c_void_p), 0, fake, None, None, 0, None, 1, fake, fake, 8, None)
        assert rc != 0 and b"observation and mask" in lib.dposer_last_error()
    finally:
        lib.dposer_scorefc_destroy(h)
    assert lib.dposer_abi_version() == 1


def test_pc_sampler_routes_probability_flow_to_the_fused_entry():
    from dposer_amd.algorithms.advanced import sampling, sde_lib
    from dposer_amd.algorithms.advanced.model import ScoreModelFC
    from dposer_amd.configs import load_config
    cfg = load_config("configs.subvp.amass_scorefc_continuous.get_config")
    m = ScoreModelFC(cfg, n_poses=21, pose_dim=3, hidden_dim=1024, embed_dim=512, n_blocks=2)
    EM, NONE, LANG = sampling.EulerMaruyamaPredictor, sampling.NoneCorrector, sampling.LangevinCorrector
    for sde, cont in ((sde_lib.subVPSDE(0.1, 20.0, 8), True), (sde_lib.VPSDE(0.1, 20.0, 8), True), (sde_lib.VPSDE(0.1, 20.0, 8), False),
                      (sde_lib.VESDE(0.01, 50.0, 8), True), (sde_lib.VESDE(0.01, 50.0, 8), False)):
        assert sampling.fused_em_supported(sde, m, EM, NONE, True, cont)
        assert sampling.fused_em_supported(sde, m, EM, None, True, cont)
        assert not sampling.fused_langevin_supported(sde, m, EM, LANG, True, cont)     # PF + corrector: the generic loop (demo.py:442)
    assert not sampling.fused_em_supported(sde_lib.subVPSDE(0.1, 20.0, 8), m, sampling.ReverseDiffusionPredictor, NONE, True, True)
