"""GPU tests of dposer_guided_sampler / sampling.get_guided_sampler: the MCG and DPS completion loops in one library call.

  forced    teacher-forced N = 1000 runs: every index stepped by the float64 oracle (tests/guided_ref.py) from the library's own state
            after the index before, inside the project's single-guided-step bounds (tests/test_gpu_score.py's golden g16 test)
  parity    golden g33 (the reference's own update_fn_guide loop; tests/test_guided_sampler_cpu.py pins the oracle loop to it and the
            oracle's fp32 run to its float64 run) at the TOLS of tests/test_gpu_pc_sampler.py -- DESIGN §2's bound for sampler outputs
  shapes, grad_step = 0 is the plain sampler, norm == 0, bit identity, sub-ranges, routing, the non-finite flag, argument checks,
  evaluate_completion's solver switch
"""
import ctypes as C

import numpy as np
import pytest
import torch

import guided_ref as G
from gpu_common import DEV, make_model, t2n
from helpers import load, rel_err

pytestmark = pytest.mark.gpu
torch.set_num_threads(8)
TOLS = {"fp32": 1e-4, "bf16x3": 1e-4, "bf16": 1e-2}          # after the 1000-step sampler (tests/test_gpu_pc_sampler.py)
STEP_TOLS = {"fp32": 1e-5, "bf16x3": 2e-5, "bf16": 2e-2}     # one guided step (tests/test_gpu_score.py, golden g16)
_MODELS = {}
INT_MAX = 2 ** 31 - 1


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device=DEV)


def _model(seed, prec):
    if (seed, prec) not in _MODELS:
        _MODELS[(seed, prec)] = make_model(seed, precision=prec)
    return _MODELS[(seed, prec)]


def _sde(kind, N):
    from dposer_amd.algorithms.advanced import sde_lib
    return (sde_lib.subVPSDE if kind == "subvp" else sde_lib.VPSDE)(0.1, 20.0, N)


def _inputs(B, seed, method, n_run, D=63):
    """x0, observation (legs replaced by noise), mask (0 on the legs), injected draws."""
    from dposer_amd.utils.misc import mask_indices
    rs = np.random.RandomState(seed)
    x0 = rs.standard_normal((B, D)).astype(np.float32)
    obs = (0.5 * rs.standard_normal((B, D))).astype(np.float32)
    mask = np.ones((B, D), np.float32)
    mask[:, mask_indices("legs", 3).numpy()] = 0.0
    noise = rs.standard_normal((n_run, G.noise_slots(method), B, D)).astype(np.float32)
    return x0, obs, mask, noise


def _run(m, kind, N, x0, obs, mask, *, method, grad_step=0.7, noise=None, seed=0, start_step=0, run_steps=-1, stride=1):
    from dposer_amd.algorithms.advanced import sampling
    sde = _sde(kind, N)
    return sampling.fused_guided_sample(m, sde, _dev(x0), torch.linspace(sde.T, 1e-3, N), _dev(obs), _dev(mask), method=method, grad_step=grad_step,
                                        start_step=start_step, run_steps=run_steps, noise=None if noise is None else _dev(noise), seed=seed,
                                        traj_stride=stride)


# ---- 1. teacher-forced whole grid ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec,every", [("fp32", 1), ("bf16x3", 50), ("bf16", 50)])
@pytest.mark.parametrize("method", G.METHODS)
@pytest.mark.parametrize("kind", ["subvp", "vp"])
def test_every_index_of_a_whole_run_against_the_float64_oracle(kind, method, prec, every):
    N, B = 1000, 5
    cfg, m, p = _model(33, prec)
    x0, obs, mask, noise = _inputs(B, 71, method, N)
    traj, x, x_mean = _run(m, kind, N, x0, obs, mask, method=method, noise=noise)
    assert torch.isfinite(traj).all() and torch.equal(x, traj[-1])                # x on return has the bits of the last trajectory entry
    got = t2n(traj)
    idx = np.arange(0, N, every)
    states = np.concatenate([x0[None], got[:-1]])[idx]                            # ahead of index i: the library's own state after i - 1
    osde = G.oracle_sde(kind, N)
    worst, where = 0.0, -1
    for k, i in enumerate(idx):
        want, _, wm = G.guided_loop(p, osde, torch.tensor(states[k], dtype=torch.float64), noise[i:i + 1], obs, mask, method=method, grad_step=0.7,
                                    start_step=int(i), run_steps=1)
        e = rel_err(got[i], want[0].numpy())
        if e > worst:
            worst, where = e, int(i)
        if i == N - 1:
            assert rel_err(t2n(x_mean), wm.numpy()) <= STEP_TOLS[prec]
    print(f"{kind} {method} {prec}: worst index {where}, rel-L2 {worst:.2e} (bound {STEP_TOLS[prec]:.0e}), max |x| {np.abs(got).max():.3g}")
    assert worst <= STEP_TOLS[prec]


# ---- 2. parity with the reference (golden g33) ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp32", "bf16x3", "bf16"])
@pytest.mark.parametrize("tag", G.golden_cases())
def test_parity_with_the_reference(tag, prec):
    from dposer_amd.algorithms.advanced import sampling
    g = load("g33_guided_sampler")
    q = G.case_inputs(g, tag)
    cfg, m, p = _model(int(g["seed"]), prec)
    fn = sampling.get_guided_sampler(_sde(q["kind"], q["N"]), (q["B"], 63), lambda v: v, q["method"], grad_step=q["grad_step"], denoise=True,
                                     eps=q["eps"], device=DEV)
    trajs, x_mean = fn(m, _dev(q["obs"]), _dev(q["mask"]), z=_dev(q["x0"]), start_step=q["start"], noise=_dev(q["noise"]), traj_stride=q["keep"])
    assert trajs.shape == g[f"{tag}_trajs"].shape
    errs = dict(final=rel_err(t2n(trajs[-1]), g[f"{tag}_final"]), x_mean=rel_err(t2n(x_mean), g[f"{tag}_final_mean"]),
                trajs=max(rel_err(a, b) for a, b in zip(t2n(trajs), g[f"{tag}_trajs"])))
    print(f"{tag} {prec}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert max(errs.values()) < TOLS[prec]


# ---- 3. shapes ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [300, 1])
def test_ragged_and_single_row_batches(B):
    """B = 300: ragged rows in the second 256-row tile, more than one block of the norm's partial sums; B = 1; D = 63: the last quad partly valid."""
    N = 12
    cfg, m, p = _model(33, "fp32")
    x0, obs, mask, noise = _inputs(B, 72 + B, "mcg", N)
    traj, x, x_mean = _run(m, "subvp", N, x0, obs, mask, method="mcg", noise=noise)
    want, wx, wm = G.guided_loop(p, G.oracle_sde("subvp", N), torch.tensor(x0, dtype=torch.float64), noise, obs, mask, method="mcg", grad_step=0.7)
    errs = [rel_err(a, b) for a, b in zip(t2n(traj), want.numpy())] + [rel_err(t2n(x_mean), wm.numpy())]
    print(f"B = {B}: worst rel-L2 {max(errs):.2e}")
    assert max(errs) < TOLS["fp32"]


# ---- 4. grad_step = 0 is the plain sampler; norm == 0 -----------------------------------------------------------------------------------------
def test_zero_grad_step_is_the_plain_sampler_and_a_zero_norm_gives_a_zero_gradient():
    from dposer_amd.algorithms.advanced import sampling
    N, B, seed = 40, 300, 12345
    cfg, m, p = _model(35, "fp32")
    x0, obs, mask, _ = _inputs(B, 73, "dps", N)
    t0, a, am = _run(m, "subvp", N, x0, obs, mask, method="dps", grad_step=0.0, seed=seed)
    sde = _sde("subvp", N)
    _, b, bm = sampling.fused_em_sample(m, sde, _dev(x0), torch.linspace(sde.T, 1e-3, N), seed=seed)      # same Philox stream and index
    e, em = rel_err(t2n(a), t2n(b)), rel_err(t2n(am), t2n(bm))
    print(f"grad_step = 0 vs dposer_em_sampler: x {e:.2e}, x_mean {em:.2e}")
    assert e < TOLS["fp32"] and em < TOLS["fp32"]
    # mask = 0 everywhere: r = 0, norm = 0 -> the gradient is 0, not 0 / 0
    t1, c, cm = _run(m, "subvp", N, x0, obs, np.zeros_like(mask), method="dps", grad_step=0.7, seed=seed)
    assert torch.isfinite(t1).all() and torch.equal(t1, t0) and torch.equal(c, a) and torch.equal(cm, am)


# ---- 5. bit identity --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", G.METHODS)
def test_repeated_and_split_runs_give_the_same_bits(method):
    N, k, B = 32, 13, 300
    cfg, m, p = _model(35, "fp32")
    x0, obs, mask, noise = _inputs(B, 74, method, N)
    for kw in (dict(noise=noise), dict(seed=99)):
        a = _run(m, "vp", N, x0, obs, mask, method=method, **kw)
        b = _run(m, "vp", N, x0, obs, mask, method=method, **kw)
        for u, v in zip(a, b):
            assert torch.isfinite(u).all() and torch.equal(u, v)
        head = {k_: (v[:k] if k_ == "noise" else v) for k_, v in kw.items()}
        tail = {k_: (v[k:] if k_ == "noise" else v) for k_, v in kw.items()}
        t1, x1, _ = _run(m, "vp", N, x0, obs, mask, method=method, run_steps=k, **head)
        t2, x2, xm2 = _run(m, "vp", N, t2n(x1), obs, mask, method=method, start_step=k, **tail)
        assert t1.shape == (k, B, 63) and torch.equal(torch.cat([t1, t2]), a[0]) and torch.equal(x2, a[1]) and torch.equal(xm2, a[2])
    c = _run(m, "vp", N, x0, obs, mask, method=method, seed=100)
    assert not torch.equal(c[1], a[1])                                         # another seed: other draws


# ---- 6. routing ---------------------------------------------------------------------------------------------------------------------------------
class _Counting:
    def __init__(self, lib, calls):
        self._lib, self._calls = lib, calls

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*a):
            self._calls.append(name)
            return fn(*a)

        return call


class _Wrapped(torch.nn.Module):
    """The same network behind a module that is not a ScoreModelFC: the pair the one-call path does not take."""

    def __init__(self, inner):
        super().__init__()
        self.inner = inner

    def forward(self, x, labels, condition=None, mask=None):
        return self.inner(x, labels)


@pytest.mark.parametrize("method", G.METHODS)
def test_the_supported_pair_is_one_library_call(method, monkeypatch):
    from dposer_amd.algorithms.advanced import sampling
    N, B = 12, 8
    cfg, m, p = _model(36, "fp32")
    x0, obs, mask, noise = _inputs(B, 75, method, N)
    fn = sampling.get_guided_sampler(_sde("subvp", N), (B, 63), lambda v: v, method, grad_step=0.7, denoise=False, device=DEV)
    args = (_dev(obs), _dev(mask))
    eng = m._engine()
    eng.packed(m.flat_params(), with_backward=True, force=True)
    m.freeze_packed, keep = True, m.freeze_packed
    calls = []
    monkeypatch.setattr(eng, "lib", _Counting(eng.lib, calls))
    m.train()
    try:
        trajs, x = fn(m, *args, z=_dev(x0), noise=_dev(noise))
        assert m.training
    finally:
        m.eval()
        m.freeze_packed = keep
        monkeypatch.undo()
    heavy = [c for c in calls if any(s in c for s in ("sampler", "forward", "backward", "langevin", "prior", "dsm"))]
    assert heavy == ["dposer_guided_sampler"], calls
    assert all(q.grad is None for q in m.parameters())
    assert trajs.shape == (N, B, 63) and torch.equal(x, trajs[-1])
    # a model outside the one-call path: the generic loop over update_fn_guide, the same numbers
    t2, x2 = fn(_Wrapped(m), *args, z=_dev(x0), noise=_dev(noise))
    e = max(rel_err(t2n(a), t2n(b)) for a, b in zip(t2, trajs))
    print(f"{method}: generic loop vs one call, worst index rel-L2 {e:.2e}")
    assert e < TOLS["fp32"] and all(q.grad is None for q in m.parameters())


# ---- 7. the non-finite flag ---------------------------------------------------------------------------------------------------------------------
def test_a_non_finite_gradient_raises_after_the_loop():
    from dposer_amd.algorithms.advanced import sampling
    N, B = 12, 8
    cfg, m, p = _model(36, "fp32")
    x0, obs, mask, noise = _inputs(B, 76, "dps", N)
    col = int(np.argmax(mask[2]))
    assert mask[2, col] == 1.0
    obs[2, col] = np.inf                                                       # an observed entry: r, the norm and the gradient are not finite
    fn = sampling.get_guided_sampler(_sde("subvp", N), (B, 63), lambda v: v, "dps", grad_step=0.7, device=DEV)
    with pytest.raises(ValueError, match=r"Consider reduce the value of parameter: grad_step=0\.7.*index 0\b"):
        fn(m, _dev(obs), _dev(mask), z=_dev(x0), noise=_dev(noise))
    assert not m.training                                                      # (eval before the call, restored although it raised)
    obs[2, col] = 0.0
    trajs, x = fn(m, _dev(obs), _dev(mask), z=_dev(x0), noise=_dev(noise))     # the next call is unaffected
    assert torch.isfinite(trajs).all()


# ---- 8. argument checks launch nothing ------------------------------------------------------------------------------------------------------------
def test_argument_checks_launch_nothing():
    from dposer_amd import _C
    from dposer_amd.algorithms.advanced import sampling, sde_lib
    N, B = 12, 8
    cfg, m, p = _model(36, "fp32")
    x0, obs, mask, noise = _inputs(B, 77, "mcg", N)
    fn = sampling.get_guided_sampler(_sde("subvp", N), (B, 63), lambda v: v, "mcg", device=DEV)
    with pytest.raises(_C.DPoserHipError):
        fn(m, torch.tensor(obs), torch.tensor(mask), z=_dev(x0))
    with pytest.raises(_C.DPoserHipError):
        fn(m, _dev(obs), _dev(mask), z=torch.tensor(x0))
    with pytest.raises(ValueError, match="shape"):
        fn(m, _dev(obs)[:4], _dev(mask)[:4], z=_dev(x0))
    with pytest.raises(ValueError, match="noise"):
        fn(m, _dev(obs), _dev(mask), z=_dev(x0), noise=_dev(noise)[:, :1])
    with pytest.raises(ValueError, match="observation and a mask"):
        fn(m, _dev(obs), None, z=_dev(x0))
    with pytest.raises(ValueError, match="method"):
        sampling.get_guided_sampler(_sde("subvp", N), (B, 63), lambda v: v, "ddrm", device=DEV)
    # the C entry: its place in the argument-check family
    eng, flat = m._engine(), m.flat_params()
    packed = eng.packed(flat, with_backward=True, force=True)
    ws = eng.workspace(B, _C.WS_GUIDED, N, torch.device(DEV))
    freq = eng.freq(torch.device(DEV), m._fourier_W())
    ts = torch.linspace(1.0, 1e-3, N).numpy()
    obs_d, mask_d = _dev(obs), _dev(mask)
    flag = torch.full((1,), INT_MAX, dtype=torch.int32, device=DEV)
    lib = _C.lib()
    ok = dict(kind="subvp", start=0, n=-1, obs=obs_d, mask=mask_d, stride=1, project=1, flag=flag, batch=B)
    cases = [(dict(obs=None), b"observation and mask"), (dict(mask=None), b"observation and mask"), (dict(start=N + 1), b"step range"),
             (dict(start=-1), b"step range"), (dict(stride=0), b"traj_stride"), (dict(project=2), b"project"), (dict(flag=None), b"nonfinite_step"),
             (dict(kind="ve"), b"sub-VP and VP"), (dict(batch=0), b"batch")]
    for kw, text in cases:
        a = dict(ok, **kw)
        sde = sde_lib.VESDE(0.01, 50.0, N) if a["kind"] == "ve" else _sde(a["kind"], N)
        x, xm = _dev(x0), torch.full((B, 63), 7.0, device=DEV)
        _C.profile_enable(True)
        rc = lib.dposer_guided_sampler(eng.h, _C.ptr(flat), _C.ptr(packed), _C.ptr(ws), C.byref(sde_lib.sde_desc(sde, True)), _C.ptr(x), _C.ptr(xm),
                                       C.c_void_p(ts.ctypes.data), a["start"], a["n"], _C.ptr(a["obs"]), _C.ptr(a["mask"]), None, 0, None, a["stride"],
                                       a["project"], 0.7, _C.ptr(a["flag"]), _C.ptr(freq), _C.ptr(m.sigmas), a["batch"], _C.stream_ptr())
        torch.cuda.synchronize()
        stats = _C.profile_collect()
        _C.profile_enable(False)
        assert rc != 0 and text in lib.dposer_last_error(), (kw, lib.dposer_last_error())
        assert torch.equal(x, _dev(x0)) and bool((xm == 7.0).all()) and not stats and int(flag.item()) == INT_MAX, (kw, stats)


# ---- 9. evaluate_completion's solvers -----------------------------------------------------------------------------------------------------------
def test_evaluate_completion_solvers():
    from dposer_amd.body_model.body_model import BodyModel
    from dposer_amd.body_model.synthetic import make_synthetic_smplx_asset
    from dposer_amd.dataset.AMASS import Posenormalizer
    from dposer_amd.tasks.completion import evaluate_completion
    cfg, m, p = _model(64, "bf16")
    bm = BodyModel(make_synthetic_smplx_asset(seed=0)).to(DEV)
    g = load("g10_normalizer")
    stats = {k.split("/")[-1]: torch.tensor(g[k]) for k in g.files if k.startswith("stats/axis_normalize")}
    nz = Posenormalizer(stats, device=DEV, normalize=True, min_max=False, rot_rep="axis")
    poses = torch.tensor(g["norm_minmax0"][:64])
    assert poses.shape[0] == 64
    sde = _sde("subvp", 24)
    for solver in ("scoresde", "mcg", "dps"):
        torch.manual_seed(5)
        means, done = evaluate_completion(m, sde, nz, bm, poses, part="legs", batch_size=32, solver=solver,
                                          solver_kwargs=dict(grad_step=0.5) if solver != "scoresde" else None)
        print(solver, means)
        assert done == 64 and set(means) == {"mpvpe_all", "mpjpe_body"} and all(np.isfinite(v) and v > 0 for v in means.values()), (solver, means)
    with pytest.raises(ValueError, match="solver"):
        evaluate_completion(m, sde, nz, bm, poses, part="legs", batch_size=32, solver="ddnm")
    # the default path: argument for argument what it was
    sde = _sde("subvp", 1000)
    kw = dict(iterations=1, steps_per_iter=3)
    outs = []
    for extra in ({}, dict(solver="dposer")):
        torch.manual_seed(5)
        m._rng_seed = 777
        outs.append(evaluate_completion(m, sde, nz, bm, poses, part="legs", batch_size=32, optimize_kwargs=kw, **extra))
    assert outs[0][1] == outs[1][1] == 64 and all(outs[0][0][k] == outs[1][0][k] for k in outs[0][0])
