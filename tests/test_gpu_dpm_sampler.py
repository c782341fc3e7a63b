"""GPU tests of the few-step sampler (dposer_dpm_sampler / sampling.get_dpm_sampler): DPM-Solver++ orders 1 and 2 in one library call.

  parity      trajectories, final state and x0_hat against the float64 statement tests/dpm_ref.py (on the fp32 times the call sees), in all
              three precisions, on sub-VP / VP / VE, both orders, the logSNR and time-uniform grids, n = 6 (start-up step, second-order
              middle, lower-order final step), 1 and 2, and the shapes that cover a partial tile, a single row, a batch across a tile
              boundary and Dpad != D; one Fourier-embedding case.  Tolerances: DESIGN §2's post-sampler figures.
  history     the oracle's own order-1 and order-2 results differ by far more than the tolerance: a kernel that ignores `hist` cannot pass
              both; lower_order_final changes the last step only
  completion  injected noise against the oracle, the wrapper's clean blend, in-kernel Philox: same seed same bits, another seed other draws
  buffers     hist needs no initialisation (NaN-filled = zero-filled, bit for bit); guard words behind x, hist, x0_hat and traj
  routing     get_sampling_fn, evaluate_completion, the generation trajectory, interpolate(decoder=...), the discrete-SDE refusal
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import dpm_ref
from gpu_common import DEV, make_model, t2n
from helpers import load, rel_err
from oracle import score_ref as R

pytestmark = pytest.mark.gpu
torch.set_num_threads(8)
TOLS = {"fp32": 1e-4, "bf16x3": 1e-4, "bf16": 1e-2}          # after a sampler loop (the fp32 oracle alone sits at <= 2.4e-6)
PRECS = ("fp32", "bf16x3", "bf16")
KINDS = ("subvp", "vp", "ve")
_MODELS = {}


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device=DEV)


def _model(prec, D=63, embedding="positional", seed=31):
    key = (seed, prec, D, embedding)
    if key not in _MODELS:
        _MODELS[key] = make_model(seed, D=D, precision=prec, embedding=embedding)
    return _MODELS[key]


def _sdes(kind, continuous=True):
    """(the library's SDE object, the oracle's)."""
    from dposer_amd.algorithms.advanced import sde_lib
    if kind == "ve":
        return sde_lib.VESDE(0.01, 50.0, 1000), R.VE(discrete=not continuous)
    if kind == "vp":
        return sde_lib.VPSDE(0.1, 20.0, 1000), R.VP(discrete=not continuous)
    return sde_lib.subVPSDE(0.1, 20.0, 1000), R.SubVP()


def _times(kind, n, grid):
    """The grid as the fp32 times of the call, widened: what the library's schedule and the oracle both see."""
    from dposer_amd.algorithms.advanced.sampling import dpm_time_grid
    return dpm_time_grid(_sdes(kind)[0], n, grid, 1e-3).astype(np.float32).astype(np.float64)


def _inputs(kind, B, D, n, seed=8):
    """x at s_0 (VE: scaled by 50, as the sampler tests do), observation / mask of a left-leg completion, imputation draws."""
    from dposer_amd.utils.misc import create_mask
    rs = np.random.RandomState(seed + 7 * B + D)
    x0 = (rs.standard_normal((B, D)) * (50.0 if kind == "ve" else 1.0)).astype(np.float32)
    mask, obs = create_mask(torch.tensor((0.5 * rs.standard_normal((B, D))).astype(np.float32)), part="left_leg")
    obs = obs * mask                                               # (create_mask draws the hidden entries from torch's generator: nothing reads them)
    noise = rs.standard_normal((n, B, D)).astype(np.float32)
    return x0, obs.numpy(), mask.numpy(), noise


@functools.lru_cache(maxsize=None)
def _oracle(kind, order, grid, B, D, n, lof=True, completion=False, embedding="positional"):
    """The float64 oracle run of one case, computed once and shared by the precisions: (trajs, x, x0_hat) as numpy."""
    _, _, p = _model("fp32", D, embedding)
    p64 = {k: v.double() for k, v in p.items()}
    x0, obs, mask, noise = _inputs(kind, B, D, n)
    kw = dict(observation=torch.tensor(obs, dtype=torch.float64), mask=torch.tensor(mask, dtype=torch.float64),
              noise=torch.tensor(noise, dtype=torch.float64)) if completion else {}
    fw = dict(embedding_type="fourier") if embedding == "fourier" else {}
    tr, x, d = dpm_ref.dpm_sampler(p64, _sdes(kind)[1], torch.tensor(x0, dtype=torch.float64), _times(kind, n, grid), order, lof, **kw, **fw)
    return tr.numpy(), x.numpy(), d.numpy()


def _run(prec, kind, order, grid, B, D, n, lof=True, completion=False, embedding="positional", noise="injected", seed=0, stride=1):
    from dposer_amd.algorithms.advanced import sampling
    _, m, _ = _model(prec, D, embedding)
    x0, obs, mask, nz = _inputs(kind, B, D, n)
    kw = dict(observation=_dev(obs), mask=_dev(mask), noise=_dev(nz) if noise == "injected" else None) if completion else {}
    return sampling.fused_dpm_sample(m, _sdes(kind)[0], _dev(x0), _times(kind, n, grid), order=order, lower_order_final=lof, seed=seed,
                                     traj_stride=stride, **kw)


def _check(got, want, tol, what):
    errs = [rel_err(t2n(g), w) for g, w in zip(got, want)]        # (each value goes to DPOSER_LOG_ERR)
    print(f"[{what}] rel-L2 trajs {errs[0]:.2e}  x {errs[1]:.2e}  x0_hat {errs[2]:.2e}  (tolerance {tol:.0e})")
    assert all(torch.isfinite(g).all() for g in got), what
    assert max(errs) < tol, (what, errs)


# ---- parity ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("grid", ["logSNR", "time_uniform"])
def test_parity_six_steps(grid, order, kind, prec):
    B, D, n = 40, 63, 6
    got = _run(prec, kind, order, grid, B, D, n)
    assert got[0].shape == (n, B, D) and torch.equal(got[0][-1], got[1])
    _check(got, _oracle(kind, order, grid, B, D, n), TOLS[prec], f"{prec} {kind} order {order} {grid} n {n}")


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,D", [(1, 63), (300, 63), (40, 126)])
def test_parity_shapes(B, D, kind, prec):
    """A single row, a batch that crosses a tile boundary, Dpad != D (order 2, logSNR grid, n = 6)."""
    got = _run(prec, kind, 2, "logSNR", B, D, 6)
    assert got[0].shape == (6, B, D)
    _check(got, _oracle(kind, 2, "logSNR", B, D, 6), TOLS[prec], f"{prec} {kind} B {B} D {D}")


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("n", [1, 2])
def test_parity_one_and_two_steps(n, order, kind, prec):
    """n = 1: the start-up step is also the last; n = 2 at order 2: with lower_order_final both steps run at order 1, without it the second
    is a second-order step."""
    for lof in (True, False):
        got = _run(prec, kind, order, "logSNR", 40, 63, n, lof=lof)
        _check(got, _oracle(kind, order, "logSNR", 40, 63, n, lof), TOLS[prec], f"{prec} {kind} order {order} n {n} lof {lof}")


def test_parity_fourier_embedding():
    got = _run("fp32", "ve", 2, "logSNR", 40, 63, 6, embedding="fourier")
    # (Fourier: sin / cos of arguments up to ~1e3, the bound of the existing Fourier cases: tests/test_gpu_pf_sampler.py)
    _check(got, _oracle("ve", 2, "logSNR", 40, 63, 6, embedding="fourier"), 2e-3, "fp32 ve fourier")


# ---- the history is really used --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("grid", ["logSNR", "time_uniform"])
def test_orders_differ_far_beyond_the_tolerance_on_the_oracle(kind, grid):
    """For the n = 6 inputs of test_parity_six_steps the oracle's order-1 and order-2 results are more than 100 x 1e-4 apart (measured:
    0.08 ... 0.18 rel-L2, i.e. also 8 ... 18 x the bf16 tolerance): no kernel can be inside the tolerance of both, so one that ignores
    `hist` fails one of the two orders."""
    o1, o2 = _oracle(kind, 1, grid, 40, 63, 6), _oracle(kind, 2, grid, 40, 63, 6)
    for a, b, what in zip(o1, o2, ("trajs", "x", "x0_hat")):
        d = rel_err(a, b)
        print(f"[{kind} {grid}] order 1 vs order 2 on the oracle, {what}: {d:.3f}")
        assert d > 100 * TOLS["fp32"]
        assert d > 2 * TOLS["bf16"]


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_lower_order_final_changes_only_the_last_step(prec):
    n = 6
    a = _run(prec, "subvp", 2, "logSNR", 40, 63, n, lof=True)
    b = _run(prec, "subvp", 2, "logSNR", 40, 63, n, lof=False)
    assert torch.equal(a[0][:n - 1], b[0][:n - 1])                 # equal through step n - 1, bit for bit
    assert not torch.equal(a[0][n - 1], b[0][n - 1])
    assert torch.equal(a[2], b[2])                                 # x0_hat = D_{n-1}: formed before the last combination
    _check(b, _oracle("subvp", 2, "logSNR", 40, 63, n, False), TOLS[prec], f"{prec} lower_order_final off")


def test_trajectory_stride():
    full = _run("fp32", "vp", 2, "logSNR", 40, 63, 6)
    for stride, want in ((2, [1, 3, 5]), (3, [2, 5]), (4, [3])):
        tr, x, d = _run("fp32", "vp", 2, "logSNR", 40, 63, 6, stride=stride)
        assert tr.shape[0] == len(want) and torch.equal(tr, full[0][want]) and torch.equal(x, full[1]) and torch.equal(d, full[2])
    tr, x, _ = _run("fp32", "vp", 2, "logSNR", 40, 63, 6, stride=0)
    assert tr is None and torch.equal(x, full[1])


# ---- completion ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("order", [1, 2])
def test_completion_parity_with_injected_noise(order, kind, prec):
    got = _run(prec, kind, order, "logSNR", 40, 63, 6, completion=True)
    _check(got, _oracle(kind, order, "logSNR", 40, 63, 6, completion=True), TOLS[prec], f"{prec} {kind} order {order} completion")


def test_completion_wrapper_blend_and_philox_streams():
    from dposer_amd.algorithms.advanced import sampling
    _, m, _ = _model("fp32")
    B, D, n = 40, 63, 6
    sde = _sdes("subvp")[0]
    x0, obs, mask, nz = _inputs("subvp", B, D, n)
    x0, obs, mask = _dev(x0), _dev(obs), _dev(mask)
    assert 0 < int((mask == 0).sum()) < mask.numel()
    for denoise in (False, True):
        fn = sampling.get_dpm_sampler(sde, (B, D), lambda v: v, steps=n, order=2, denoise=denoise, device=DEV)
        trajs, out = fn(m, observation=obs, mask=mask, z=x0, noise=_dev(nz))
        raw = _run("fp32", "subvp", 2, "logSNR", B, D, n, completion=True)
        assert trajs.shape == (n, B, D) and torch.equal(trajs, raw[0])
        assert torch.equal(out[mask == 1], obs[mask == 1])         # the observed entries are the observation, bit for bit
        assert torch.equal(out[mask == 0], (raw[2] if denoise else raw[1])[mask == 0])
    fn = sampling.get_dpm_sampler(sde, (B, D), lambda v: v, steps=n, order=2, device=DEV)
    t1, o1 = fn(m, observation=obs, mask=mask, z=x0, seed=11)
    t2, o2 = fn(m, observation=obs, mask=mask, z=x0, seed=11)
    t3, o3 = fn(m, observation=obs, mask=mask, z=x0, seed=12)
    assert torch.equal(t1, t2) and torch.equal(o1, o2)             # one seed: the same bits
    assert torch.isfinite(t3).all()
    sel = (mask == 1).expand_as(t1)
    assert not torch.equal(t1[sel], t3[sel])                       # another seed: other imputation draws on the mask
    assert float((t1[sel] != t3[sel]).float().mean()) > 0.99
    with pytest.raises(ValueError, match="go together"):
        fn(m, observation=obs, z=x0)


# ---- buffer safety ---------------------------------------------------------------------------------------------------------------------
GUARD = 64
SENTINEL = -12345.5


def _raw_call(prec, kind, order, n, B, D, hist_fill, traj_stride=1):
    """dposer_dpm_sampler on caller buffers with guard words behind x, hist, x0_hat and traj."""
    from dposer_amd import _C
    from dposer_amd.algorithms.advanced import sde_lib
    _, m, _ = _model(prec, D)
    sde = _sdes(kind)[0]
    x0, _, _, _ = _inputs(kind, B, D, n)
    eng, flat = m._engine(), m.flat_params()
    packed = eng.packed(flat, with_backward=False, force=True)
    ws = eng.workspace(B, _C.WS_SHARED_T, n, torch.device(DEV))

    def guarded(numel, fill):
        buf = torch.full((numel + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
        buf[:numel] = fill
        return buf

    n_traj = n // traj_stride
    x, hist, x0_hat, traj = guarded(B * D, 0.0), guarded(B * D, hist_fill), guarded(B * D, 7.0), guarded(n_traj * B * D, 7.0)
    x[:B * D] = _dev(x0).reshape(-1)
    ts = torch.tensor(_times(kind, n, "logSNR"), dtype=torch.float32)
    desc, dpm = sde_lib.sde_desc(sde, True), _C.DpmDesc(order, 1)
    _C.check(eng.lib.dposer_dpm_sampler(eng.h, _C.ptr(flat), _C.ptr(packed), _C.ptr(ws), C.byref(desc), C.byref(dpm), _C.ptr(x), _C.ptr(x0_hat),
                                        _C.ptr(hist), C.c_void_p(ts.data_ptr()), n, None, None, None, 0, _C.ptr(traj), traj_stride,
                                        _C.ptr(eng.freq(torch.device(DEV), m._fourier_W())), _C.ptr(m.sigmas), B, _C.stream_ptr()), "dposer_dpm_sampler")
    torch.cuda.synchronize()
    for name, buf, numel in (("x", x, B * D), ("hist", hist, B * D), ("x0_hat", x0_hat, B * D), ("traj", traj, n_traj * B * D)):
        assert bool((buf[numel:] == SENTINEL).all()), f"guard words behind {name} were written"
    return x[:B * D].clone(), x0_hat[:B * D].clone(), traj[:n_traj * B * D].clone(), hist[:B * D].clone()


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("B,D", [(40, 63), (300, 63), (1, 126)])
def test_hist_needs_no_initialisation_and_guards_stay_intact(B, D, order, prec):
    n = 6
    a = _raw_call(prec, "subvp", order, n, B, D, float("nan"))
    b = _raw_call(prec, "subvp", order, n, B, D, 0.0)
    for u, v in zip(a, b):
        assert torch.isfinite(u).all() and torch.equal(u, v)
    assert torch.equal(a[1], a[3])                                 # hist ends as the last data prediction = x0_hat
    ref = _run(prec, "subvp", order, "logSNR", B, D, n)
    assert torch.equal(a[0].reshape(B, D), ref[1]) and torch.equal(a[2].reshape(n, B, D), ref[0])
    _raw_call(prec, "subvp", order, n, B, D, float("nan"), traj_stride=4)      # one slot for six steps: nothing lands behind it


# ---- routing ---------------------------------------------------------------------------------------------------------------------------
def test_get_sampling_fn_routes_dpm():
    from dposer_amd.algorithms.advanced import sampling
    cfg, m, _ = _model("fp32")
    sde = _sdes("subvp")[0]
    B = 40
    x0 = _dev(_inputs("subvp", B, 63, 6)[0])
    old = dict(cfg.sampling)
    try:
        cfg.sampling.method = "dpm"
        cfg.sampling.dpm_steps, cfg.sampling.dpm_order, cfg.sampling.dpm_skip_type = 6, 2, "logSNR"
        cfg.sampling.noise_removal = False
        trajs, x = sampling.get_sampling_fn(cfg, sde, (B, 63), lambda v: v, 1e-3, device=DEV)(m, z=x0)
        raw = _run("fp32", "subvp", 2, "logSNR", B, 63, 6)
        assert trajs.shape == (6, B, 63) and torch.equal(trajs, raw[0]) and torch.equal(x, raw[1])
        cfg.sampling.noise_removal = True
        _, d = sampling.get_sampling_fn(cfg, sde, (B, 63), lambda v: v, 1e-3, device=DEV)(m, z=x0)
        assert torch.equal(d, raw[2])                              # denoise: the last data prediction
        for k in ("dpm_steps", "dpm_order", "dpm_skip_type"):      # the defaults: 20 steps, order 2, logSNR
            del cfg.sampling[k]
        trajs, _ = sampling.get_sampling_fn(cfg, sde, (B, 63), lambda v: v, 1e-3, device=DEV)(m, z=x0)
        assert trajs.shape == (20, B, 63) and torch.isfinite(trajs).all()
        cfg.sampling.method = "dpm++"
        with pytest.raises(ValueError, match="Sampler name dpm\\+\\+ unknown"):
            sampling.get_sampling_fn(cfg, sde, (B, 63), lambda v: v, 1e-3, device=DEV)
    finally:
        cfg.sampling.clear()
        cfg.sampling.update(old)


def _normalizer():
    from dposer_amd.dataset.AMASS import Posenormalizer
    g = load("g10_normalizer")
    stats = {k.split("/")[-1]: torch.tensor(g[k]) for k in g.files if k.startswith("stats/axis_normalize")}
    return g, Posenormalizer(stats, device=DEV, normalize=True, min_max=False, rot_rep="axis")


def test_evaluate_completion_with_the_dpm_solver():
    from dposer_amd.body_model.body_model import BodyModel
    from dposer_amd.body_model.synthetic import make_synthetic_smplx_asset
    from dposer_amd.tasks.completion import SOLVERS, evaluate_completion
    assert "dpm" in SOLVERS
    _, m, _ = _model("bf16", seed=64)
    bm = BodyModel(make_synthetic_smplx_asset(seed=0)).to(DEV)
    g, nz = _normalizer()
    poses = torch.tensor(g["norm_minmax0"][:64])
    sde = _sdes("subvp")[0]
    res = []
    for seed in (3, 3, 4):
        torch.manual_seed(5)
        means, done = evaluate_completion(m, sde, nz, bm, poses, part="left_leg", hypo=2, batch_size=32, solver="dpm",
                                          solver_kwargs=dict(steps=8, order=2, skip_type="logSNR", eps=1e-3, seed=seed))
        print("dpm", seed, means)
        assert done == 64 and set(means) == {"mpvpe_all", "mpjpe_body"} and all(np.isfinite(v) and v > 0 for v in means.values()), means
        res.append(means)
    assert res[0] == res[1] and res[0] != res[2]                   # the seed keys the hypotheses' draws


def test_generation_keeps_every_state_of_the_few_step_solver(tmp_path):
    from dposer_amd.body_model.body_model import BodyModel
    from dposer_amd.body_model.synthetic import make_synthetic_smplx_asset
    from dposer_amd.tasks.generation import generation_process
    from dposer_amd.utils.motion_video import read_video
    cfg, m, _ = _model("fp32")
    bm = BodyModel(make_synthetic_smplx_asset(seed=0)).to(DEV)
    _, nz = _normalizer()
    old = dict(cfg.sampling)
    try:
        cfg.sampling.method, cfg.sampling.dpm_steps = "dpm", 7
        torch.manual_seed(0)
        paths = generation_process(m, _sdes("subvp")[0], cfg, nz, bm, str(tmp_path / "gen"), video_num=2)
    finally:
        cfg.sampling.clear()
        cfg.sampling.update(old)
    assert len(paths) == 2
    for q in paths:
        video, fps = read_video(q)
        assert video.shape == (7, 512, 384, 3) and fps == 30.0    # one frame per solver step


def test_interpolate_decoder_switch():
    from dposer_amd.tasks import interpolation as I
    _, m, _ = _model("fp32", seed=34)
    sde = _sdes("subvp")[0]
    rs = np.random.RandomState(9)
    anchors = _dev(rs.standard_normal((3, 63)) * 0.8)
    epsilon = _dev(rs.choice([-1.0, 1.0], size=(3, 63)))
    kw = dict(frames=5, encode_kw=dict(epsilon=epsilon))
    z0, r0, f0 = I.interpolate(m, sde, anchors, **kw)
    z1, r1, f1 = I.interpolate(m, sde, anchors, decoder="pf", **kw)
    assert torch.equal(z0, z1) and torch.equal(r0, r1) and torch.equal(f0, f1)      # "pf" is the default, bit for bit
    z2, r2, f2 = I.interpolate(m, sde, anchors, decoder="dpm", decoder_kw=dict(steps=10), **kw)
    assert torch.equal(z2, z0) and r2.shape == (3, 63) and f2.shape == (2, 5, 63)
    assert torch.isfinite(r2).all() and torch.isfinite(f2).all()
    assert torch.equal(f2[:, 0], r2[:-1]) or rel_err(t2n(f2[:, 0]), t2n(r2[:-1])) < 1e-4      # segment ends decode the anchors' latents
    with pytest.raises(ValueError, match="decoder"):
        I.interpolate(m, sde, anchors, decoder="ddim", **kw)


def test_discrete_score_functions_are_refused():
    from dposer_amd import _C
    from dposer_amd.algorithms.advanced import sampling
    _, m, _ = _model("fp32")
    x0 = _dev(_inputs("vp", 40, 63, 6)[0])
    for kind in ("vp", "ve"):
        fn = sampling.get_dpm_sampler(_sdes(kind)[0], (40, 63), lambda v: v, steps=6, continuous=False, device=DEV)
        with pytest.raises(_C.DPoserHipError, match="code -2"):
            fn(m, z=x0)
    # the entry itself refuses before it launches: x is untouched
    from dposer_amd.algorithms.advanced import sde_lib
    sde = _sdes("vp")[0]
    eng, flat = m._engine(), m.flat_params()
    packed = eng.packed(flat, with_backward=False, force=True)
    ws = eng.workspace(40, _C.WS_SHARED_T, 6, torch.device(DEV))
    x, hist = x0.clone(), torch.zeros_like(x0)
    ts = torch.tensor(_times("vp", 6, "logSNR"), dtype=torch.float32)
    for desc, dpm, code in ((sde_lib.sde_desc(sde, False), _C.DpmDesc(2, 1), -2), (sde_lib.sde_desc(sde, True), _C.DpmDesc(3, 1), -1)):
        rc = eng.lib.dposer_dpm_sampler(eng.h, _C.ptr(flat), _C.ptr(packed), _C.ptr(ws), C.byref(desc), C.byref(dpm), _C.ptr(x), None, _C.ptr(hist),
                                        C.c_void_p(ts.data_ptr()), 6, None, None, None, 0, None, 1,
                                        _C.ptr(eng.freq(torch.device(DEV), m._fourier_W())), _C.ptr(m.sigmas), 40, _C.stream_ptr())
        torch.cuda.synchronize()
        assert rc == code and torch.equal(x, x0)
