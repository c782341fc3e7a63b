"""GPU tests of dposer_pc_sampler: every registered predictor and corrector of pc_sampler in one library call.

  band      one step per call behind the constant-output network (tests/test_gpu_sde_sweep.py's method, restated), against the float64
            stages of tests/pc_ref.py: |kernel - ref64| <= the derived fp32 band, per element, x_mean and x; all five SDE kinds, with
            and without scale_by_sigma, plain and completion (mask values 0, 1, 0.25, 0.625).  A measured ratio near 1 on x_mean is
            the final addition's own rounding (sde_ref.langevin explains).  In-kernel draws are regenerated from oracle/philox.py.
  parity    get_sampling_fn against golden g32 (the reference's own Predictor / Corrector objects; tests/test_pc_sampler_cpu.py pins the
            oracle loop to it) at the TOLS of tests/test_gpu_pf_sampler.py -- DESIGN §2's bound for sampler outputs
  identity  (Euler-Maruyama, none) and (Euler-Maruyama, langevin) give the bits of dposer_em_sampler / fused_pc_langevin_sample
  whole     teacher-forced N = 1000 runs (reverse_diffusion + ald with completion, ancestral_sampling + none) inside the band at every index
  routing, argument checks, sub-ranges
"""
import ctypes as C

import numpy as np
import pytest
import torch

import pc_ref as P
import sde_ref as S
from gpu_common import DEV, make_model, t2n
from helpers import _log_measured, load, rel_err
from pc_ref import case_inputs, golden_cases as _cases, parse_tag

pytestmark = pytest.mark.gpu
torch.set_num_threads(8)
TOLS = {"fp32": 1e-4, "bf16x3": 1e-4, "bf16": 1e-2}          # after the 1000-step sampler (tests/test_gpu_pf_sampler.py)
_MODELS = {}
CASES = [(k, 1000, sc) for k in S.KINDS for sc in (True, False)]
SNR = 0.16


def _ids(cases):
    return [f"{k}-N{n}-{'scaled' if sc else 'raw'}" for k, n, sc in cases]


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device=DEV)


def _sde(kind, N):
    from dposer_amd.algorithms.advanced import sde_lib
    if kind.startswith("ve"):
        return sde_lib.VESDE(sigma_min=0.01, sigma_max=50.0, N=N)
    return (sde_lib.subVPSDE if kind == "subvp" else sde_lib.VPSDE)(0.1, 20.0, N)


class _Args:
    def __init__(self, task):
        self.task = task


# ---- the constant-output network and the band (restated from tests/test_gpu_sde_sweep.py) ----------------------------------------------
def _c(D, seed=11):
    rs = np.random.RandomState(seed)
    return (rs.choice([-1.0, 1.0], D) * np.exp(rs.uniform(np.log(1e-2), np.log(4.0), D))).astype(np.float32)


def _model(D, scale):
    """post_dense.weight = 0, post_dense.bias = c: the raw network output is c bit for bit (asserted)."""
    from dposer_amd import _C
    if D not in _MODELS:
        cfg, m, p = make_model(41, D=D, precision="fp32")
        c = _c(D)
        with torch.no_grad():
            m.post_dense.weight.zero_()
            m.post_dense.bias.copy_(torch.tensor(c))
        _C.bump_param_epoch()
        _MODELS[D] = (m, c)
    m, c = _MODELS[D]
    m.config.model.scale_by_sigma = False
    m._engines.clear()
    rs = np.random.RandomState(5)
    with torch.no_grad():
        raw = m(torch.tensor(rs.standard_normal((7, D)).astype(np.float32), device=DEV),
                torch.tensor(rs.uniform(1.0, 998.0, 7).astype(np.float32), device=DEV))
    assert raw.cpu().numpy().tobytes() == np.broadcast_to(c, (7, D)).astype(np.float32).tobytes()
    m.config.model.scale_by_sigma = scale
    m._engines.clear()
    return m, c


def _times(N=1000, every=1):
    grids = np.concatenate([torch.linspace(1.0, 1e-3, 1000).numpy()[::every], torch.linspace(1.0, 1e-5, 1000).numpy()[::every]])
    edge = [S.boundary_times(999), S.boundary_times(N - 1), S.half_times(N), np.asarray([1.0, 1e-5, 1e-3], np.float32)]
    return np.unique(np.concatenate([grids] + edge).astype(np.float32))


def _refs(kind, N, scale, t32, fn):
    """fn(scalars, used_sigma, table entries) for each admissible sigma index (two under the continuous VE kind: test_gpu_sde_sweep._refs)."""
    sig = load("g8_scalars")["sigmas_buffer"]
    table = load("g27_vp_tables")[f"sqrt_1m_alphas_cumprod_{N}"] if kind == "vp_discrete" else None
    s = S._col(S.scalars(kind, t32, N=N, table=table), 2)
    lab = s["label"]
    if not isinstance(lab, S.E) and np.ndim(lab):
        lab = lab[(Ellipsis, None, None)]
    tb = P.table_entries(kind, t32, N, _table_np(kind, N))
    tb = {k: (v[..., None, None] if isinstance(v, S.E) else v) for k, v in tb.items()}
    sides = (-1, 1) if (kind == "ve" and scale) else (0,)
    return [fn(s, S.used_sigma(sig, lab, False, scale, side), tb) for side in sides]


def _judge(name, got, refs, t32=None):
    r = S.ratio_any(got, refs)
    w = float(r.max()) if r.size else 0.0
    _log_measured("band_ratio_" + name, w)
    where = np.unravel_index(int(np.argmax(r)), r.shape) if r.size else ()
    at = "" if t32 is None or not where else f" at t = {float(np.asarray(t32).reshape(-1)[where[0]])!r}"
    print(f"{name}: worst band ratio {w:.3f}{at} (index {where})")
    assert w <= 1.0, f"{name}: worst band ratio {w:.3f}{at}, element {where}"


def _drawn_normals(rows, cols, stream, offset, seed):
    """rng.h normals4 as float64 values of the same Philox bits with the 5.5-ulp band of the fp32 Box-Muller (test_gpu_sde_sweep._drawn_normals)."""
    from oracle import philox as PH
    qd = (cols + 3) // 4
    idx = (np.arange(rows, dtype=np.uint64)[:, None] * np.uint64(qd) + np.arange(qd, dtype=np.uint64)[None, :]).reshape(-1)
    r = PH.philox4x32_10((idx & np.uint64(0xFFFFFFFF)).astype(np.uint32), (idx >> np.uint64(32)).astype(np.uint32), np.uint32(stream),
                         np.uint32(offset), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    out = []
    for a, b in ((r[0], r[1]), (r[2], r[3])):
        rad = np.sqrt(-2.0 * np.log(PH.u01_open_low(a).astype(np.float64)))
        ang = (np.float32(2.0 * np.pi) * PH.u01(b)).astype(np.float64)
        out += [rad * np.cos(ang), rad * np.sin(ang)]
    z = np.stack(out, axis=-1).reshape(rows, qd * 4)[:, :cols]
    return S.E(z, 5.5 * S.ULP * np.abs(z))


def _table_np(kind, N):
    from dposer_amd.algorithms.advanced import sampling
    return sampling._discrete_table(_sde(kind, N)).numpy()


class _Call:
    """Everything of a raw dposer_pc_sampler call on model m."""

    def __init__(self, m, kind, N, B, rows=1):
        from dposer_amd import _C
        from dposer_amd.algorithms.advanced import sde_lib
        self.m, self.B = m, B
        self.eng = m._engine()
        self.flat = m.flat_params()
        self.packed = self.eng.packed(self.flat, with_backward=False, force=True)
        self.ws = self.eng.workspace(B, _C.WS_SHARED_T, rows, torch.device(DEV))
        self.freq = self.eng.freq(torch.device(DEV), m._fourier_W())
        self.desc = sde_lib.sde_desc(_sde(kind, N), kind in ("subvp", "vp", "ve"))
        self.table = np.ascontiguousarray(_table_np(kind, N), dtype=np.float32)
        self.norms = torch.zeros(2, device=DEV)

    def __call__(self, pred, corr, x, x_mean, ts, t_off, start, n_steps, *, n_each=1, pf=0, obs=None, mask=None, noise=None, seed=0, traj=None,
                 stride=1, table=True, norms=True, check=True):
        from dposer_amd import _C
        pc = _C.PcDesc(pred, corr, n_each, pf, SNR, 1.0 / self.B)
        rc = self.eng.lib.dposer_pc_sampler(self.eng.h, _C.ptr(self.flat), _C.ptr(self.packed), _C.ptr(self.ws), C.byref(self.desc), C.byref(pc),
                                            _C.ptr(x), _C.ptr(x_mean), C.c_void_p(ts.ctypes.data + 4 * t_off), start, n_steps, _C.ptr(obs),
                                            _C.ptr(mask), _C.ptr(noise), seed, _C.ptr(traj), stride,
                                            C.c_void_p(self.table.ctypes.data) if table else None, _C.ptr(self.norms) if norms else None,
                                            _C.ptr(self.freq), _C.ptr(self.m.sigmas), self.B, _C.stream_ptr())
        if check:
            _C.check(rc, "dposer_pc_sampler")
        return rc


def _data(B, D, seed, scale=1.0):
    rs = np.random.RandomState(seed)
    return [(rs.standard_normal((B, D)) * (scale if i == 0 else 1.0)).astype(np.float32) for i in range(5)]


def _stage_sweep(what, kind, N, scale, B, D, t32, completion):
    """One loop index per call from a fresh x with injected noise.  what = a predictor (corrector 'none': imputation ahead of the predictor,
    the predictor, imputation after it) or 'ald' (predictor 'none': ALD, the imputation after the corrector fused into its kernel,
    x_mean = x, imputation after the predictor)."""
    from dposer_amd import _C
    m, c = _model(D, scale)
    call = _Call(m, kind, N, B)
    x, z, obs, zb, za = _data(B, D, 300 + B, 50.0 if kind.startswith("ve") else 1.0)
    mask = np.random.RandomState(302).choice(np.asarray([0.0, 1.0, 0.25, 0.625], np.float32), size=(B, D))
    G = len(t32)
    xs = _dev(np.broadcast_to(x, (G, B, D)).copy())
    means = torch.empty((G, B, D), device=DEV)
    ald = what == "ald"
    if completion:
        noise = _dev(np.stack([z, za, z, zb]) if ald else np.stack([za, z, zb]))
    else:
        noise = _dev(np.stack([z, z]) if ald else z[None])
    obs_d, mask_d = (_dev(obs), _dev(mask)) if completion else (None, None)
    ts = np.ascontiguousarray(t32, dtype=np.float32)
    pred = {"ald": _C.PC_PRED_NONE, "none": _C.PC_PRED_NONE, "reverse_diffusion": _C.PC_PRED_REVERSE_DIFFUSION,
            "ancestral_sampling": _C.PC_PRED_ANCESTRAL}[what]
    for i in range(G):
        call(pred, _C.PC_CORR_ALD if ald else _C.PC_CORR_NONE, xs[i], means[i], ts, i, 0, 1, obs=obs_d, mask=mask_d, noise=noise)

    def ref(s, us, tb):
        score = P.score_of(kind, s, us, c[None, None, :])
        o, mk = (obs[None], mask[None]) if completion else (None, None)
        if ald:
            a = P.ald_stage(kind, s, tb, score, x[None], z[None], SNR, obs=o, mask=mk, z_imp=za[None] if completion else None)["x"]
            return dict(x_mean=a, x=P._impute(s, a, o, mk, zb[None]) if completion else a)
        x_in = S.E(x[None])
        if completion:
            x_in = P._impute(s, x_in, o, mk, za[None])
        return P.predictor_stage(what, kind, s, tb, score, x_in, z[None], N, obs=o, mask=mk, z_imp_b=zb[None] if completion else None)

    refs = _refs(kind, N, scale, t32, ref)
    name = f"pc_{what}_{'completion' if completion else 'plain'}_{kind}_N{N}_{'scaled' if scale else 'raw'}_B{B}_D{D}"
    _judge(f"{name}_x_mean", means.cpu().numpy(), [r["x_mean"] for r in refs], t32)
    _judge(f"{name}_x", xs.cpu().numpy(), [r["x"] for r in refs], t32)


def _defined(what, kind):
    return not (what == "ancestral_sampling" and kind == "subvp")


WHATS = ("reverse_diffusion", "ancestral_sampling", "none", "ald")
# (ancestral sampling is not defined on sub-VP: refused, test_argument_checks_launch_nothing)
STAGE_CASES = [(k, n, sc, w) for k, n, sc in CASES for w in WHATS if _defined(w, k)]
STAGE_IDS = [f"{i}-{w}" for i, (_, _, _, w) in zip(_ids([c_[:3] for c_ in STAGE_CASES]), STAGE_CASES)]


@pytest.mark.parametrize("completion", [False, True], ids=["plain", "completion"])
@pytest.mark.parametrize("kind,N,scale,what", STAGE_CASES, ids=STAGE_IDS)
def test_stage_on_the_whole_grid(kind, N, scale, what, completion):
    _stage_sweep(what, kind, N, scale, 5, 63, _times(N), completion)


@pytest.mark.parametrize("completion", [False, True], ids=["plain", "completion"])
@pytest.mark.parametrize("B,D", [(1, 126), (33, 126)])
@pytest.mark.parametrize("kind,N,scale,what", STAGE_CASES, ids=STAGE_IDS)
def test_stage_other_shapes(kind, N, scale, what, B, D, completion):
    """One row / 33 rows with the 2-element quad tail, every 10th time."""
    _stage_sweep(what, kind, N, scale, B, D, _times(N, every=10), completion)


def _whole_run(kind, N, scale, pred, corr, completion):
    """All N loop indices of one call on linspace(T, 1e-5, N) with a trajectory; the reference recomputes loop index i from the kernel's
    own state after i - 1 (with a corrector there is no look-ahead imputation: the recorded state is the one the next index starts
    from), so nothing accumulates and every per-step quantity the host forms -- table entry, noise slot, time-table row -- is judged
    per element at every index."""
    from dposer_amd import _C
    B, D = 5, 63
    m, c = _model(D, scale)
    call = _Call(m, kind, N, B, rows=N)
    t32 = np.ascontiguousarray(torch.linspace(1.0, 1e-5, N).numpy())
    rs = np.random.RandomState(901)
    x0 = (rs.standard_normal((B, D)) * (50.0 if kind.startswith("ve") else 1.0)).astype(np.float32)
    ald = corr == "ald"
    k_slots, s_impa, s_pred, s_impb = P.noise_slots(corr, 1, completion)
    noise = rs.standard_normal((N, k_slots, B, D)).astype(np.float32)
    obs = rs.standard_normal((B, D)).astype(np.float32)
    mask = rs.choice(np.asarray([0.0, 1.0, 0.25, 0.625], np.float32), size=(B, D))
    x, x_mean, traj = _dev(x0), torch.empty((B, D), device=DEV), torch.empty((N, B, D), device=DEV)
    obs_d, mask_d = (_dev(obs), _dev(mask)) if completion else (None, None)
    call({"reverse_diffusion": _C.PC_PRED_REVERSE_DIFFUSION, "ancestral_sampling": _C.PC_PRED_ANCESTRAL}[pred],
         _C.PC_CORR_ALD if ald else _C.PC_CORR_NONE, x, x_mean, t32, 0, 0, -1, obs=obs_d, mask=mask_d, noise=_dev(noise), traj=traj)
    got = traj.cpu().numpy()
    assert np.isfinite(got).all()
    prev = np.concatenate([x0[None], got[:-1]])                     # the kernel's own state ahead of every loop index

    def ref(s, us, tb):
        score = P.score_of(kind, s, us, c[None, None, :])
        o, mk = (obs[None], mask[None]) if completion else (None, None)
        x_in = S.E(prev)
        if ald:
            x_in = P.ald_stage(kind, s, tb, score, x_in, noise[:, 0], SNR, obs=o, mask=mk, z_imp=noise[:, s_impa] if completion else None)["x"]
        elif completion:
            x_in = P._impute(s, x_in, o, mk, noise[:, s_impa])
        return P.predictor_stage(pred, kind, s, tb, score, x_in, noise[:, s_pred], N, obs=o, mask=mk, z_imp_b=noise[:, s_impb] if completion else None)

    refs = _refs(kind, N, scale, t32, ref)
    name = f"pc_run_{pred}_{corr}_{kind}_N{N}_{'scaled' if scale else 'raw'}"
    _judge(f"{name}_traj", got, [r["x"] for r in refs], t32)
    _judge(f"{name}_x_mean_last", x_mean.cpu().numpy(), [r["x_mean"][-1] for r in refs])
    assert x.cpu().numpy().tobytes() == got[-1].tobytes()


@pytest.mark.parametrize("kind,N,scale", CASES, ids=_ids(CASES))
def test_whole_run_teacher_forced_reverse_diffusion_ald_completion(kind, N, scale):
    _whole_run(kind, N, scale, "reverse_diffusion", "ald", True)


ANC_CASES = [c_ for c_ in CASES if c_[0] != "subvp"]


@pytest.mark.parametrize("kind,N,scale", ANC_CASES, ids=_ids(ANC_CASES))
def test_whole_run_teacher_forced_ancestral_none(kind, N, scale):
    """Corrector 'none' without an observation: no imputation at all, the recorded state is the next index's input."""
    _whole_run(kind, N, scale, "ancestral_sampling", "none", False)


@pytest.mark.parametrize("pf_kind", ["subvp", "vp", "ve"])
def test_reverse_diffusion_probability_flow_step(pf_kind):
    """The full score term (factor 1) and G = 0: x == x_mean; the predictor slot is present and not read."""
    from dposer_amd import _C
    N, B, D = 1000, 5, 63
    m, c = _model(D, True)
    call = _Call(m, pf_kind, N, B)
    x = _data(B, D, 310, 50.0 if pf_kind == "ve" else 1.0)[0]
    t32 = _times(N, every=10)
    xs, means = _dev(np.broadcast_to(x, (len(t32), B, D)).copy()), torch.empty((len(t32), B, D), device=DEV)
    noise = torch.full((1, B, D), 1e3, device=DEV)
    for i in range(len(t32)):
        call(_C.PC_PRED_REVERSE_DIFFUSION, _C.PC_CORR_NONE, xs[i], means[i], t32, i, 0, 1, pf=1, noise=noise)
    refs = _refs(pf_kind, N, True, t32, lambda s, us, tb: P.predictor_stage("reverse_diffusion", pf_kind, s, tb, P.score_of(pf_kind, s, us, c[None, None, :]),
                                                                            x[None], None, N, pf=True))
    _judge(f"pc_rd_pf_{pf_kind}_x_mean", means.cpu().numpy(), [r["x_mean"] for r in refs], t32)
    assert torch.equal(xs, means)


BIG_T = np.asarray([1.0, 0.5005005, 1e-3], np.float32)


@pytest.mark.parametrize("completion", [False, True], ids=["plain", "completion"])
@pytest.mark.parametrize("what,kind", [("reverse_diffusion", "subvp"), ("ancestral_sampling", "vp"), ("ald", "ve")])
def test_in_kernel_draws(what, kind, completion):
    """noise = None: one loop index at each of three t (start_step = 0, 1, 2 of a three-entry time list, so the Philox offset is the loop
    index i): STREAM_EM_NOISE at i for the predictors, STREAM_LANGEVIN at i * n_steps_each + k for ALD; with an observation
    STREAM_IMPUTE_A at i (ahead of the predictor: the stand-alone launch, or fused into ALD's last inner step) and STREAM_IMPUTE_B at i."""
    from dposer_amd import _C
    from oracle import philox as PH
    N, B, D, seed = 1000, 33, 63, 77
    m, c = _model(D, True)
    call = _Call(m, kind, N, B)
    x, obs = _data(B, D, 1200 + B, 50.0 if kind == "ve" else 1.0)[:2]
    mask = np.random.RandomState(303).choice(np.asarray([0.0, 1.0, 0.25, 0.625], np.float32), size=(B, D))
    obs_d, mask_d = (_dev(obs), _dev(mask)) if completion else (None, None)
    G = len(BIG_T)
    xs, means = _dev(np.broadcast_to(x, (G, B, D)).copy()), torch.empty((G, B, D), device=DEV)
    ald = what == "ald"
    pred = _C.PC_PRED_NONE if ald else (_C.PC_PRED_REVERSE_DIFFUSION if what == "reverse_diffusion" else _C.PC_PRED_ANCESTRAL)
    for i in range(G):
        call(pred, _C.PC_CORR_ALD if ald else _C.PC_CORR_NONE, xs[i], means[i], BIG_T, 0, i, 1, seed=seed, obs=obs_d, mask=mask_d)

    def drawn(stream):
        zs = [_drawn_normals(B, D, stream, i, seed) for i in range(G)]
        return S.E(np.stack([a.v for a in zs]), np.stack([a.e for a in zs]))

    z, za, zb = drawn(PH.STREAM_LANGEVIN if ald else PH.STREAM_EM_NOISE), drawn(PH.STREAM_IMPUTE_A), drawn(PH.STREAM_IMPUTE_B)

    def ref(s, us, tb):
        score = P.score_of(kind, s, us, c[None, None, :])
        o, mk = (obs[None], mask[None]) if completion else (None, None)
        if ald:
            a = P.ald_stage(kind, s, tb, score, x[None], z, SNR, obs=o, mask=mk, z_imp=za if completion else None)
            return dict(x_mean=a["x"], x=P._impute(s, a["x"], o, mk, zb) if completion else a["x"])
        x_in = P._impute(s, S.E(x[None]), o, mk, za) if completion else x[None]
        return P.predictor_stage(what, kind, s, tb, score, x_in, z, N, obs=o, mask=mk, z_imp_b=zb if completion else None)

    refs = _refs(kind, N, True, BIG_T, ref)
    name = f"pc_drawn_{what}_{kind}_{'completion' if completion else 'plain'}"
    _judge(f"{name}_x", xs.cpu().numpy(), [r["x"] for r in refs], BIG_T)
    _judge(f"{name}_x_mean", means.cpu().numpy(), [r["x_mean"] for r in refs], BIG_T)


# ---- parity with the reference's own objects (golden g32) ------------------------------------------------------------------------------------
def _golden_run(g, tag, prec):
    from dposer_amd.algorithms.advanced import sampling
    c, q = parse_tag(tag), case_inputs(g, tag)
    cfg, m, p = make_model(int(g["seed"]), precision=prec)
    cfg.sampling.predictor, cfg.sampling.corrector = c["predictor"], c["corrector"]
    cfg.sampling.n_steps_each, cfg.sampling.snr, cfg.sampling.probability_flow = q["n_each"], float(g["snr"]), c["pf"]
    cfg.training.continuous = True
    fn = sampling.get_sampling_fn(cfg, _sde(c["kind"], q["N"]), (q["B"], 63), lambda v: v, q["eps"], device=DEV)
    # the draws in the slots of the library's noise argument: regenerated in the reference's order
    rs = np.random.RandomState(int(g["noise_seed"]))
    k_slots, s_impa, s_pred, s_impb = P.noise_slots(c["corrector"], q["n_each"], c["completion"])
    n_run = q["N"] - q["start"]
    noise = np.zeros((n_run, k_slots, q["B"], 63), np.float32)
    draws = 0
    for i in range(n_run):
        slots = list(range(0 if c["corrector"] == "none" else q["n_each"])) + ([s_impa] if c["completion"] else [])
        slots += ([s_pred] if c["predictor"] != "none" else []) + ([s_impb] if c["completion"] else [])
        for s_ in slots:
            noise[i, s_] = rs.standard_normal((q["B"], 63)).astype(np.float32)
            draws += 1
    assert draws == q["n_draws"]
    kw = {}
    if c["completion"]:
        kw = dict(observation=_dev(g[f"{tag}_obs"]), mask=_dev(g[f"{tag}_mask"]), args=_Args("completion"))
    elif q["start"]:
        kw = dict(start_step=q["start"], args=_Args("denoise"))
    trajs, x = fn(m, z=_dev(q["z0"]), noise=_dev(noise), traj_stride=q["keep"], **kw)
    return trajs, x, q


@pytest.mark.parametrize("tag", _cases())
def test_parity_with_the_reference_fp32(tag):
    g = load("g32_pc_variants")
    trajs, x, q = _golden_run(g, tag, "fp32")
    e = rel_err(t2n(x), g[f"{tag}_final"])
    print(f"{tag}: final rel-L2 {e:.2e}")
    assert e < TOLS["fp32"]
    if f"{tag}_trajs" in g.files:
        et = rel_err(t2n(trajs), g[f"{tag}_trajs"])
        print(f"{tag}: trajectory rel-L2 {et:.2e}")
        assert trajs.shape == g[f"{tag}_trajs"].shape and et < TOLS["fp32"]


@pytest.mark.parametrize("prec", ["bf16x3", "bf16"])
@pytest.mark.parametrize("tag", [t for t in _cases() if "N1000" in t or "completion" in t or "denoise" in t or "anc_none" in t or "lang" in t])
def test_parity_with_the_reference_bf16(tag, prec):
    g = load("g32_pc_variants")
    trajs, x, q = _golden_run(g, tag, prec)
    e, et = rel_err(t2n(x), g[f"{tag}_final"]), rel_err(t2n(trajs), g[f"{tag}_trajs"])
    print(f"{tag} {prec}: final rel-L2 {e:.2e}, trajectory {et:.2e}")
    assert e < TOLS[prec] and et < TOLS[prec]


# ---- bit identity where nothing may change ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_euler_maruyama_pairs_keep_their_bits(prec):
    from dposer_amd.algorithms.advanced import sampling
    cfg, m, p = make_model(35, precision=prec)
    N, B = 40, 300                                                         # Bpad past one 256-row tile
    sde = _sde("subvp", N)
    z0 = torch.randn(B, 63, device=DEV, generator=torch.Generator(device=DEV).manual_seed(6))
    ts = torch.linspace(sde.T, 1e-3, N)
    EM, NONE, LANG = sampling.EulerMaruyamaPredictor, sampling.NoneCorrector, sampling.LangevinCorrector
    a = sampling.fused_em_sample(m, sde, z0, ts, seed=9, traj_stride=1)
    b = sampling.fused_pc_sample(m, sde, z0, ts, predictor=EM, corrector=NONE, seed=9, traj_stride=1)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    rs = np.random.RandomState(10)
    obs, mask = _dev(rs.standard_normal((B, 63))), _dev(rs.choice([0.0, 1.0, 0.25, 0.625], size=(B, 63)))
    inj = torch.randn(N, 5, B, 63, device=DEV, generator=torch.Generator(device=DEV).manual_seed(11))
    # plain; completion (the stand-alone imputation launch after the corrector); completion with injected draws, two corrector steps
    for kw in (dict(n_steps=1), dict(n_steps=1, observation=obs, mask=mask), dict(n_steps=2, observation=obs, mask=mask, noise=inj)):
        a = sampling.fused_pc_langevin_sample(m, sde, z0, ts, snr=SNR, seed=9, traj_stride=1, **kw)
        b = sampling.fused_pc_sample(m, sde, z0, ts, predictor=EM, corrector=LANG, snr=SNR, seed=9, traj_stride=1, **kw)
        for name, u, v in zip(("traj", "x", "x_mean"), a, b):
            assert torch.isfinite(u).all() and torch.equal(u, v), (sorted(kw), name, rel_err(t2n(v), t2n(u)))
    o = dict(observation=obs, mask=mask)
    a = sampling.fused_em_sample(m, sde, z0, ts, seed=9, traj_stride=1, **o)
    b = sampling.fused_pc_sample(m, sde, z0, ts, predictor=EM, corrector=NONE, seed=9, traj_stride=1, **o)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


# ---- routing ------------------------------------------------------------------------------------------------------------------------------------
def test_every_supported_pair_is_one_library_call(monkeypatch):
    from dposer_amd.algorithms.advanced import sampling

    def boom(*a, **k):
        raise AssertionError("generic loop reached")

    monkeypatch.setattr(sampling, "shared_predictor_update_fn", boom)
    monkeypatch.setattr(sampling, "shared_corrector_update_fn", boom)
    calls = []
    real = sampling.fused_pc_sample
    monkeypatch.setattr(sampling, "fused_pc_sample", lambda *a, **k: calls.append(1) or real(*a, **k))
    cfg, m, p = make_model(36, precision="bf16")
    B, N = 16, 32
    n = 0
    for kind in ("subvp", "vp", "ve"):
        z0 = torch.randn(B, 63, device=DEV, generator=torch.Generator(device=DEV).manual_seed(7)) * (50.0 if kind == "ve" else 1.0)
        for pred in ("none", "euler_maruyama", "reverse_diffusion", "ancestral_sampling"):
            for corr in ("none", "ald", "langevin"):
                if (pred, corr) == ("euler_maruyama", "none") or (pred == "ancestral_sampling" and kind == "subvp"):
                    continue
                cfg.sampling.predictor, cfg.sampling.corrector, cfg.sampling.probability_flow = pred, corr, False
                fn = sampling.get_sampling_fn(cfg, _sde(kind, N), (B, 63), lambda v: v, 1e-3, device=DEV)
                trajs, x = fn(m, z=z0, seed=3)
                n += 1
                assert len(calls) == n and torch.isfinite(x).all() and trajs.shape == (N, B, 63), (kind, pred, corr)
                if corr == "ald" and pred == "reverse_diffusion":
                    _, x2 = fn(m, z=z0, seed=3)
                    _, x3 = fn(m, z=z0, seed=4)
                    n += 2
                    assert torch.equal(x, x2) and not torch.equal(x, x3)       # one seed: the same bits; another: not
    cfg.sampling.predictor, cfg.sampling.corrector, cfg.sampling.probability_flow = "reverse_diffusion", "none", True
    fn = sampling.get_sampling_fn(cfg, _sde("subvp", N), (B, 63), lambda v: v, 1e-3, device=DEV)
    _, x = fn(m, z=z0)
    assert len(calls) == n + 1 and torch.isfinite(x).all()
    cfg.sampling.corrector = "ald"                                          # PF + corrector stays on the generic loop
    fn = sampling.get_sampling_fn(cfg, _sde("subvp", N), (B, 63), lambda v: v, 1e-3, device=DEV)
    with pytest.raises(AssertionError, match="generic loop reached"):
        fn(m, z=z0)
    assert len(calls) == n + 1


# ---- argument checks and sub-ranges ---------------------------------------------------------------------------------------------------------------
def test_argument_checks_launch_nothing():
    from dposer_amd import _C
    cfg, m, p = make_model(37, precision="fp32")
    B, N = 8, 32
    x0 = torch.randn(B, 63, device=DEV)
    ts = torch.linspace(1.0, 1e-3, N).numpy()
    lib = _C.lib()
    RD, ANC, NONE, LANG, ALD = _C.PC_PRED_REVERSE_DIFFUSION, _C.PC_PRED_ANCESTRAL, _C.PC_CORR_NONE, _C.PC_CORR_LANGEVIN, _C.PC_CORR_ALD
    cases = [("subvp", ANC, NONE, {}, b"VE and VP"), ("vp", ANC, NONE, dict(pf=1), b"probability flow"), ("vp", RD, NONE, dict(table=False), b"disc_table_host"),
             ("subvp", RD, ALD, dict(table=False), b"disc_table_host"), ("ve", RD, LANG, dict(norms=False), b"norm_sums"),
             ("subvp", RD, ALD, dict(n_each=0), b"n_steps_each"), ("subvp", 7, NONE, {}, b"predictor kind")]
    for kind, pred, corr, kw, text in cases:
        call = _Call(m, kind, N, B, rows=N)
        x, xm = x0.clone(), torch.full((B, 63), 7.0, device=DEV)
        _C.profile_enable(True)
        rc = call(pred, corr, x, xm, ts, 0, 0, -1, check=False, **kw)
        torch.cuda.synchronize()
        stats = _C.profile_collect()
        _C.profile_enable(False)
        assert rc != 0 and text in lib.dposer_last_error(), (kind, pred, corr, kw, lib.dposer_last_error())
        assert torch.equal(x, x0) and bool((xm == 7.0).all()) and not stats, (kind, pred, corr, stats)
    # the three older entries share the loop and its checks
    call = _Call(m, "subvp", N, B, rows=N)
    obs = torch.zeros(B, 63, device=DEV)
    traj = torch.empty(N, B, 63, device=DEV)
    em_cases = [(e, dict(obs=obs), b"go together") for e in ("dposer_em_sampler", "dposer_pf_sampler")]
    em_cases += [("dposer_em_sampler_steps", dict(n_steps=-1), b"n_steps")]
    for e in ("dposer_em_sampler", "dposer_pf_sampler", "dposer_em_sampler_steps"):
        em_cases += [(e, dict(stride=0), b"traj_stride"), (e, dict(start=N + 1), b"step range")]
    for entry, kw, text in em_cases:
        x, xm = x0.clone(), torch.full((B, 63), 7.0, device=DEV)
        steps = (kw.get("n_steps", 1),) if entry == "dposer_em_sampler_steps" else ()
        _C.profile_enable(True)
        rc = getattr(lib, entry)(call.eng.h, _C.ptr(call.flat), _C.ptr(call.packed), _C.ptr(call.ws), C.byref(call.desc), _C.ptr(x), _C.ptr(xm),
                                 C.c_void_p(ts.ctypes.data), kw.get("start", 0), *steps, _C.ptr(kw.get("obs")), None, None, 0, _C.ptr(traj),
                                 kw.get("stride", 1), _C.ptr(call.freq), _C.ptr(m.sigmas), B, _C.stream_ptr())
        torch.cuda.synchronize()
        stats = _C.profile_collect()
        _C.profile_enable(False)
        assert rc != 0 and text in lib.dposer_last_error(), (entry, sorted(kw), lib.dposer_last_error())
        assert torch.equal(x, x0) and bool((xm == 7.0).all()) and not stats, (entry, sorted(kw), stats)


@pytest.mark.parametrize("pred,corr", [("reverse_diffusion", "ald"), ("ancestral_sampling", "none"), ("none", "langevin")])
def test_a_sub_range_gives_the_bits_of_the_whole_run(pred, corr):
    from dposer_amd.algorithms.advanced import sampling
    cfg, m, p = make_model(38, precision="fp32")
    N, B = 32, 300
    sde = _sde("vp", N)
    z0 = torch.randn(B, 63, device=DEV, generator=torch.Generator(device=DEV).manual_seed(8))
    ts = torch.linspace(sde.T, 1e-3, N)
    rs = np.random.RandomState(4)
    obs, mask = _dev(rs.standard_normal((B, 63))), _dev(rs.choice([0.0, 1.0, 0.25], size=(B, 63)))
    kw = dict(predictor=sampling.get_predictor(pred), corrector=sampling.get_corrector(corr), snr=SNR, n_steps=2, seed=5, observation=obs, mask=mask)
    traj, x, xm = sampling.fused_pc_sample(m, sde, z0, ts, traj_stride=1, **kw)
    t2, x2, xm2 = sampling.fused_pc_sample(m, sde, traj[9], ts, start_step=10, run_steps=7, traj_stride=1, **kw)
    assert t2.shape == (7, B, 63) and torch.equal(t2, traj[10:17]) and torch.equal(x2, traj[16])
    t3, x3, xm3 = sampling.fused_pc_sample(m, sde, traj[16], ts, start_step=17, traj_stride=1, **kw)
    assert torch.equal(t3, traj[17:]) and torch.equal(x3, x) and torch.equal(xm3, xm)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_an_euler_maruyama_sub_range_gives_the_bits_of_the_whole_run(prec):
    """dposer_em_sampler_steps over [4, 7) from traj[3] of a whole completion run.  B = 300: ragged rows in the second 256-row tile;
    D = 63: the last quad partly valid."""
    from dposer_amd import _C
    from dposer_amd.algorithms.advanced import sampling
    cfg, m, p = make_model(39, precision=prec)
    N, B = 12, 300
    sde = _sde("subvp", N)
    z0 = torch.randn(B, 63, device=DEV, generator=torch.Generator(device=DEV).manual_seed(12))
    ts = torch.linspace(sde.T, 1e-3, N)
    rs = np.random.RandomState(5)
    obs, mask = _dev(rs.standard_normal((B, 63))), _dev(rs.choice([0.0, 1.0, 0.25], size=(B, 63)))
    traj, _, _ = sampling.fused_em_sample(m, sde, z0, ts, seed=5, traj_stride=1, observation=obs, mask=mask)
    call = _Call(m, "subvp", N, B, rows=3)
    x, xm, t2 = traj[3].clone(), torch.empty(B, 63, device=DEV), torch.empty(3, B, 63, device=DEV)
    _C.check(call.eng.lib.dposer_em_sampler_steps(call.eng.h, _C.ptr(call.flat), _C.ptr(call.packed), _C.ptr(call.ws), C.byref(call.desc), _C.ptr(x),
                                                  _C.ptr(xm), C.c_void_p(ts.numpy().ctypes.data), 4, 3, _C.ptr(obs), _C.ptr(mask), None, 5, _C.ptr(t2),
                                                  1, _C.ptr(call.freq), _C.ptr(m.sigmas), B, _C.stream_ptr()), "dposer_em_sampler_steps")
    assert torch.equal(t2, traj[4:7])
