"""The rule of the joint-residual stage and of DPS on observed 3D joints (tests/joint_guided_ref.py) on the CPU, the `supported`
predicates of the two samplers, and what dposer_joint_guide_stage / dposer_joint_guided_sampler export and refuse without a GPU: every
refusal is an argument check (nothing is launched) and its message starts with the name of the entry that was called."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import guided_ref as G
import joint_guided_ref as jg
import rot_ref as rr
from dposer_amd import _C
from weights import make_weights
from oracle import score_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG, UNSUPPORTED = -1, -2
FAKE = C.c_void_p(0x1000)
MISALIGNED = C.c_void_p(0x1010)
TIMES = (C.c_float * 66)(*[1.0 - i / 80.0 for i in range(66)])
torch.set_num_threads(8)


def _jrest():
    a = rr.body_asset()
    return torch.tensor(a["J_regressor"].astype(np.float64) @ a["v_template"].astype(np.float64))


def _stage_kw(B, n_obs=22, rows=None, seed=0, conf=True):
    rs = np.random.RandomState(seed)
    a, b = torch.tensor(rs.standard_normal(63) * 0.1), torch.tensor(rs.uniform(0.2, 0.5, 63))
    obs = torch.tensor(rs.standard_normal((B, n_obs, 3)) * 0.3)
    c = torch.tensor(rs.uniform(0.2, 1.5, (B, n_obs))) if conf else None
    return dict(mode=1, a=a, b=b, root=torch.tensor(rs.standard_normal((B, 3)) * 0.3), transl=torch.tensor(rs.standard_normal((B, 3)) * 0.2),
                j_rest=_jrest(), obs=obs, conf=c, rows=rows)


def test_v_is_half_the_gradient_of_s_by_central_differences():
    B = 3
    kw = _stage_kw(B, n_obs=3, rows=[20, 15, 21], seed=1)
    y0 = torch.tensor(np.random.RandomState(2).standard_normal((B, 63)))
    s, v = jg.joint_stage(y0, **kw)
    h = 1e-6
    for col in (0, 7, 31, 47, 62):
        e = torch.zeros(63, dtype=torch.float64)
        e[col] = h
        fd = (jg.stage_sum(y0 + e, **kw) - jg.stage_sum(y0 - e, **kw)) / (2 * h)
        assert float((0.5 * fd - v[:, col]).abs().max()) < 1e-7 * max(1.0, float(v[:, col].abs().max()))
    assert float(v.abs().max()) > 0


def test_dead_entries_holding_nan_change_nothing():
    B = 4
    kw = _stage_kw(B, seed=3)
    y0 = torch.tensor(np.random.RandomState(4).standard_normal((B, 63)))
    dead = torch.tensor(np.random.RandomState(5).uniform(size=(B, 22)) < 0.4)
    dead[1] = True                                               # a row without a live entry
    conf0 = torch.where(dead, torch.zeros_like(kw["conf"]), kw["conf"])
    s0, v0 = jg.joint_stage(y0, **dict(kw, conf=conf0))
    for bad_c in (0.0, -2.0, float("nan")):
        conf = torch.where(dead, torch.full_like(conf0, bad_c), conf0)
        obs = torch.where(dead[..., None], torch.full_like(kw["obs"], float("nan")), kw["obs"])
        s, v = jg.joint_stage(y0, **dict(kw, conf=conf, obs=obs))
        assert bool(torch.isfinite(s).all()) and bool(torch.isfinite(v).all())
        assert torch.equal(s, s0) and torch.equal(v, v0)
    assert float(s0[1]) == 0.0 and not bool(v0[1].any())


def _loop_inputs(B, N, seed, n_obs=22):
    rs = np.random.RandomState(seed)
    p = dict(make_weights(33, D=63))
    p["sigmas"] = R.sigma_table()
    kw = _stage_kw(B, n_obs=n_obs, seed=seed + 1)
    x0 = rs.standard_normal((B, 63))
    noise = rs.standard_normal((N, 1, B, 63))
    return p, kw, x0, noise


def _loop(p, kw, x0, noise, N, rows=slice(None), dtype=torch.float64, **over):
    sl = lambda v: v[rows] if (v is not None and v.dim() >= 2 and v.shape[0] == x0.shape[0]) else v
    args = dict(mode=kw["mode"], a=kw["a"], b=kw["b"], root=sl(kw["root"]), transl=sl(kw["transl"]), j_rest=kw["j_rest"], norm="sample", grad_step=0.7,
                dtype=dtype)
    args.update(over)
    return jg.joint_guided_loop(p, G.oracle_sde("subvp", N), torch.tensor(x0[rows]), noise[:, :, rows], sl(kw["obs"]), sl(kw["conf"]), kw["rows"], **args)


def test_a_row_stepped_alone_equals_the_row_in_a_batch_of_five():
    N, B, start = 8, 5, 4
    p, kw, x0, noise = _loop_inputs(B, N - start, 11)
    full, _, _ = _loop(p, kw, x0, noise, N, start_step=start)
    one, _, _ = _loop(p, kw, x0, noise, N, rows=slice(3, 4), start_step=start)
    assert float((full[:, 3:4] - one).abs().max()) < 1e-12
    coupled, _, _ = _loop(p, kw, x0, noise, N, start_step=start, norm="batch")
    assert float((coupled[:, 3:4] - one).abs().max()) > 1e-6


def test_an_exact_fit_gives_a_zero_norm_and_a_zero_gradient():
    """All 22 joints observed at the exact FK of the current y0: s == 0 and the step is the unguided one (norm == 0 gives grad = 0)."""
    N, B = 8, 3
    p, kw, x0, noise = _loop_inputs(B, 1, 21)
    p = G.params_as(p, torch.float64)
    sde = G.oracle_sde("subvp", N)
    x = torch.tensor(x0)
    t = torch.ones(B, dtype=torch.float64) * 0.3
    _, _, score = R.rsde_sde(p, sde, x, t)
    alpha, sigma = sde.alpha_sigma(t)
    y0 = (x + (sigma ** 2)[:, None] * score) / alpha
    exact = jg.fk22(jg.denormalise(y0, kw["mode"], kw["a"], kw["b"]), kw["root"], kw["j_rest"], kw["transl"]).detach()
    stage = dict(kw, obs=exact, conf=None)
    s, v = jg.joint_stage(y0.detach(), **stage)
    assert float(s.abs().max()) == 0.0 and float(v.abs().max()) == 0.0
    z = torch.tensor(noise[0, 0])
    for norm in ("sample", "batch"):
        guided, y_mean, s2 = jg.joint_guided_step(p, sde, x, t, z, stage, norm=norm, grad_step=0.7)
        plain, pm = R.em_step(p, sde, x, t, z)
        assert float(s2.abs().max()) == 0.0 and torch.equal(guided, plain.detach()) and torch.equal(y_mean, pm.detach())


def test_the_rule_in_float32_over_the_whole_grid():
    """e32(i): the rule stepped in float32 against float64 from the same state, every 25th index of N = 1000 at B = 5 -- what the rule alone
    does, for the reader of a GPU failure.  Printed; the only assertion is that the late window meets the single-step bound."""
    N, B = 1000, 5
    idx = np.arange(0, N, 25)
    n = len(idx)
    p, kw, x0, noise = _loop_inputs(B, N, 31)
    rs = np.random.RandomState(32)
    ts = torch.linspace(1.0, 1e-3, N)
    sde = G.oracle_sde("subvp", N)
    states = rs.standard_normal((n * B, 63))                     # prior-like states at every index: the early indices are the hard ones
    tile = lambda v: v.repeat((n,) + (1,) * (v.dim() - 1))
    out = {}
    for dt in (torch.float64, torch.float32):
        stage = dict(mode=1, a=kw["a"].to(dt), b=kw["b"].to(dt), root=tile(kw["root"]).to(dt), transl=tile(kw["transl"]).to(dt), j_rest=kw["j_rest"].to(dt),
                     obs=tile(kw["obs"]).to(dt), conf=tile(kw["conf"]).to(dt), rows=None)
        xs, _, _ = jg.joint_guided_step(G.params_as(p, dt), sde, torch.tensor(states).to(dt), ts.to(dt)[idx].repeat_interleave(B),
                                        torch.tensor(noise[idx, 0].reshape(n * B, 63)).to(dt), stage, norm="sample", grad_step=0.7, group=B)
        out[dt] = xs.double().numpy().reshape(n, B, 63)
    e32 = np.array([np.linalg.norm(out[torch.float32][k] - out[torch.float64][k]) / np.linalg.norm(out[torch.float64][k]) for k in range(n)])
    print("\nindex      t      e32")
    for k in range(n):
        print(f"{idx[k]:5d}  {float(ts[idx[k]]):.3f}  {e32[k]:.2e}")
    assert np.isfinite(e32).all() and e32[ts.numpy()[idx] <= 0.2].max() < 1e-5


def test_supported_predicates():
    from dposer_amd.algorithms.advanced import sampling, sde_lib
    from dposer_amd.algorithms.advanced.model import ScoreModelFC
    from dposer_amd.configs import load_config
    cfg = load_config("configs.subvp.amass_scorefc_continuous.get_config")
    m63 = ScoreModelFC(cfg, n_poses=21, pose_dim=3, hidden_dim=64, embed_dim=32, n_blocks=2)
    m126 = ScoreModelFC(cfg, n_poses=21, pose_dim=6, hidden_dim=64, embed_dim=32, n_blocks=2)
    sub, vp, ve = sde_lib.subVPSDE(0.1, 20.0, 10), sde_lib.VPSDE(0.1, 20.0, 10), sde_lib.VESDE(0.01, 50.0, 10)
    for f in (sampling.fused_guided_supported, sampling.fused_joint_guided_supported):
        assert f(sub, m63, True) and f(vp, m63, True)
        assert not f(ve, m63, True) and not f(vp, m63, False) and not f(sub, torch.nn.Linear(3, 3), True)
    assert sampling.fused_guided_supported(sub, m126, True) and not sampling.fused_joint_guided_supported(sub, m126, True)
    with pytest.raises(ValueError, match="norm scope"):
        sampling.get_joint_guided_sampler(sub, (4, 63), None, None, norm="row")
    with pytest.raises(ValueError, match="63"):
        sampling.get_joint_guided_sampler(sub, (4, 126), None, None)


# ---- exports and refusals ------------------------------------------------------------------------------------------------------------------------
NAMES = ("dposer_fk_joints_backward", "dposer_fk_joints_backward_workspace_bytes", "dposer_joint_guide_stage", "dposer_joint_guide_stage_scratch_bytes",
         "dposer_joint_guided_sampler", "dposer_joint_guided_scratch_bytes")


def test_the_entries_are_exported_declared_and_bound():
    lib = _C.lib()
    header = open(os.path.join(ROOT, "include", "dposer_hip.h")).read()
    for name in NAMES:
        assert hasattr(lib, name) and name in _C.SIGNATURES and f" {name}(" in header, name
    assert lib.dposer_joint_guide_stage_scratch_bytes(7) == 7 * 522 * 4
    assert lib.dposer_joint_guided_scratch_bytes(7) == 7 * (522 + 127) * 4 and lib.dposer_joint_guided_scratch_bytes(0) == 0


@pytest.fixture(scope="module")
def body():
    lib = _C.lib()
    h = C.c_void_p()
    assert lib.dposer_body_create(C.byref(_C.BodyDesc(55, 1000, 10, 0, 0)), (C.c_int32 * 55)(*jg.SMPLX_PARENTS), C.byref(h)) == 0
    yield h
    lib.dposer_body_destroy(h)


@pytest.fixture(scope="module")
def nets():
    lib = _C.lib()
    hs = {}
    for D in (63, 126):
        h = C.c_void_p()
        assert lib.dposer_scorefc_create(C.byref(_C.ScoreFCDesc(D, 1024, 512, 2, _C.EMB_POSITIONAL, 1, 1000, _C.PREC_FP32, 0.1)), C.byref(h)) == 0
        hs[D] = h
    yield hs
    for h in hs.values():
        lib.dposer_scorefc_destroy(h)


def _sde(kind=_C.SDE_SUBVP):
    return C.byref(_C.SdeDesc(kind, 1000, 0.1, 20.0, 1.0))


def _stage_args(o):
    return [o["body"], FAKE, o.get("data_dim", 63), o.get("norm_mode", 1), FAKE, FAKE, None, None, FAKE, 0, FAKE, None, None, o.get("n_obs", 3), FAKE, FAKE,
            o.get("scratch", FAKE), o.get("batch", 16), None]


def _sampler_args(o):
    return [o["h"], FAKE, FAKE, o.get("ws", FAKE), o.get("sde", _sde()), FAKE, FAKE, TIMES, 0, 3, o["body"], 1, FAKE, FAKE, None, None, FAKE, 0, FAKE, None,
            None, o.get("n_obs", 3), o.get("norm_scope", 1), None, 0, None, o.get("traj_stride", 1), 1.0, FAKE, o.get("scratch", FAKE), FAKE, FAKE, 16, None]


STAGE_CASES = [
    ("null handle", {"body": None}, BAD_ARG, "null handle"),
    ("a 126-wide pose", {"data_dim": 126}, UNSUPPORTED, "rot6d"),
    ("data_dim 64", {"data_dim": 64}, BAD_ARG, "data_dim must be 63"),
    ("norm_mode 3", {"norm_mode": 3}, BAD_ARG, "bad normaliser"),
    ("n_obs 0", {"n_obs": 0}, BAD_ARG, "n_obs must be in 1..22"),
    ("n_obs 23", {"n_obs": 23}, BAD_ARG, "n_obs must be in 1..22"),
    ("empty batch", {"batch": 0}, BAD_ARG, "batch must be positive"),
    ("null scratch", {"scratch": None}, BAD_ARG, "scratch must be non-null and 16-byte aligned"),
    ("misaligned scratch", {"scratch": C.c_void_p(0x1008)}, BAD_ARG, "scratch must be non-null and 16-byte aligned"),
]
SAMPLER_CASES = [
    ("null handle", {"h": None}, BAD_ARG, "null argument"),
    ("misaligned workspace", {"ws": MISALIGNED}, BAD_ARG, "packed / workspace must be 256-byte aligned"),
    ("null sde", {"sde": None}, BAD_ARG, "null argument"),
    ("null body", {"body": None}, BAD_ARG, "body, j_rest and joints_obs are required"),
    ("VE", {"sde": _sde(_C.SDE_VE)}, UNSUPPORTED, "continuous sub-VP and VP"),
    ("VE discrete", {"sde": _sde(_C.SDE_VE_DISCRETE)}, UNSUPPORTED, "continuous sub-VP and VP"),
    ("VP discrete", {"sde": _sde(_C.SDE_VP_DISCRETE)}, UNSUPPORTED, "continuous sub-VP and VP"),
    ("sde kind 9", {"sde": _sde(9)}, BAD_ARG, "unknown SDE kind"),
    ("a 126-wide network", {"D": 126}, UNSUPPORTED, "rot6d (126) is not supported"),
    ("norm_scope 2", {"norm_scope": 2}, BAD_ARG, "norm_scope must be 0 (batch) or 1 (sample)"),
    ("norm_scope -1", {"norm_scope": -1}, BAD_ARG, "norm_scope must be 0 (batch) or 1 (sample)"),
    ("n_obs 0", {"n_obs": 0}, BAD_ARG, "n_obs must be in 1..22"),
    ("n_obs 23", {"n_obs": 23}, BAD_ARG, "n_obs must be in 1..22"),
    ("traj_stride 0", {"traj_stride": 0}, BAD_ARG, "traj_stride must be >= 1"),
    ("misaligned scratch", {"scratch": C.c_void_p(0x1008)}, BAD_ARG, "scratch must be non-null and 16-byte aligned"),
]


@pytest.mark.parametrize("what,over,code,text", STAGE_CASES, ids=[c[0].replace(" ", "_") for c in STAGE_CASES])
def test_stage_refusal(body, what, over, code, text):
    lib = _C.lib()
    o = {"body": body}
    o.update(over)
    rc = lib.dposer_joint_guide_stage(*_stage_args(o))
    msg = lib.dposer_last_error().decode()
    assert rc == code, (rc, msg)
    assert text in msg and msg.startswith("dposer_joint_guide_stage: "), msg


@pytest.mark.parametrize("what,over,code,text", SAMPLER_CASES, ids=[c[0].replace(" ", "_") for c in SAMPLER_CASES])
def test_sampler_refusal(body, nets, what, over, code, text):
    lib = _C.lib()
    o = {"body": body, "h": nets[over.get("D", 63)]}
    o.update({k: v for k, v in over.items() if k != "D"})
    rc = lib.dposer_joint_guided_sampler(*_sampler_args(o))
    msg = lib.dposer_last_error().decode()
    assert rc == code, (rc, msg)
    assert text in msg and msg.startswith("dposer_joint_guided_sampler: "), msg
