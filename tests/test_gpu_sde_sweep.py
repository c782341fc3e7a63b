"""Every kernel that consumes the SDE scalars at a time t, swept over the real time grids against the float64 reference of
tests/sde_ref.py -- per element, inside the derived fp32 band (|kernel - ref64| <= band; sde_ref's docstring has the derivation, and
tests/test_sde_ref_cpu.py validates reference and band on the CPU, seeded faults included).

The network is taken out of the comparison: post_dense.weight = 0 and post_dense.bias = c (seeded, mixed signs, |c| in [1e-2, 4]), so the
raw network output is c bit for bit -- asserted first in every case, by a forward without scale_by_sigma -- and every output is a pure
function of (t, x, z, c).  fp32 precision throughout: the band is fp32's.

Time values (`_times`): linspace(T, 1e-3, 1000) (the tasks' grid), linspace(T, 1e-5, 1000) (the samplers'), for k in {0, 1, 2, 4, 5, 499,
500, 998, 999} the two adjacent fp32 t whose fp32 product with 999 -- and with N - 1 -- falls on either side of k, t with
(T - t)(N - 1) = k + 0.5 exactly for even and odd k, t = T and t = eps: 2021 values at N = 1000.
Kinds: all five at N = 1000, and VP-discrete at N = 2000 without scale_by_sigma (labels past the 1000 sigmas).
The sigma index trunc(sigma(t)) of the continuous VE kind is decided by a powf: at t = T (sigma = 50.0) both indices are admissible,
everywhere else every index is exact (test_sde_ref_cpu.py asserts that t = T is the only such value).

Sums: the bands of the losses carry k 2^-24 sum|term| with k counted from the kernels (sde_ref.chain_blocked): k_denoise one term per
grid-stride pass, k_ddim_step / k_red_diff four, + 6 shuffle levels + 3 cross-wave additions, + k_sum_partials (<= 4 serial + 6 + 3);
k_pf_rhs_end: ceil(D / 64) serial + 6 shuffle levels; k_dsm's loss and the column sums of dres: sde_ref.dsm_chains.

Draws made in a kernel (z = None) are regenerated from oracle/philox.py as float64 values of the same Philox bits, with the band of the
fp32 Box-Muller evaluation (`_drawn_normals`); the drawn t of the training step is two rounded fp32 operations and is bit-exact.

Every worst band ratio is logged through helpers._log_measured (DPOSER_LOG_ERR).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import sde_ref as S
from gpu_common import DEV, make_model
from helpers import _log_measured, load

pytestmark = pytest.mark.gpu
torch.set_num_threads(8)

_MODELS = {}
CASES = [(k, 1000, sc) for k in S.KINDS for sc in (True, False)] + [("vp_discrete", 2000, False)]
CONT = [(k, 1000, sc) for k in ("subvp", "vp", "ve") for sc in (True, False)]


def _ids(cases):
    return [f"{k}-N{n}-{'scaled' if sc else 'raw'}" for k, n, sc in cases]


def _c(D, seed=11):
    rs = np.random.RandomState(seed)
    return (rs.choice([-1.0, 1.0], D) * np.exp(rs.uniform(np.log(1e-2), np.log(4.0), D))).astype(np.float32)


def _model(D, scale, embedding="positional"):
    """The constant-output network; asserts that its raw output is c bit for bit."""
    from dposer_amd import _C
    key = (D, scale, embedding)
    if key not in _MODELS:
        cfg, m, p = make_model(41, D=D, precision="fp32", embedding=embedding)
        c = _c(D)
        with torch.no_grad():
            m.post_dense.weight.zero_()
            m.post_dense.bias.copy_(torch.tensor(c))
        _C.bump_param_epoch()
        _MODELS[key] = (m, c)
    m, c = _MODELS[key]
    m.config.model.scale_by_sigma = False            # the raw output: an engine without the sigma division
    m._engines.clear()
    rs = np.random.RandomState(5)
    with torch.no_grad():
        raw = m(torch.tensor(rs.standard_normal((7, D)).astype(np.float32), device=DEV),
                torch.tensor(rs.uniform(1.0, 998.0, 7).astype(np.float32), device=DEV))
    assert raw.cpu().numpy().tobytes() == np.broadcast_to(c, (7, D)).astype(np.float32).tobytes()
    m.config.model.scale_by_sigma = scale
    m._engines.clear()
    return m, c


def _sde(kind, N):
    from dposer_amd.algorithms.advanced import sde_lib
    if kind.startswith("ve"):
        return sde_lib.VESDE(sigma_min=0.01, sigma_max=50.0, N=N)
    return (sde_lib.subVPSDE if kind == "subvp" else sde_lib.VPSDE)(0.1, 20.0, N)


def _desc(kind, N):
    from dposer_amd.algorithms.advanced import sde_lib
    d = sde_lib.sde_desc(_sde(kind, N), kind in ("subvp", "vp", "ve"))
    assert d is not None
    return d


def _times(N=1000, every=1):
    grids = np.concatenate([torch.linspace(1.0, 1e-3, 1000).numpy()[::every], torch.linspace(1.0, 1e-5, 1000).numpy()[::every]])
    edge = [S.boundary_times(999), S.boundary_times(N - 1), S.half_times(N), np.asarray([1.0, 1e-5, 1e-3], np.float32)]
    return np.unique(np.concatenate([grids] + edge).astype(np.float32))


def _table(kind, N):
    return load("g27_vp_tables")[f"sqrt_1m_alphas_cumprod_{N}"] if kind == "vp_discrete" else None


def _data(B, D, seed):
    rs = np.random.RandomState(seed)
    return [rs.standard_normal((B, D)).astype(np.float32) for _ in range(4)]


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a), device=DEV)


def _drawn_normals(rows, cols, stream, offset, seed):
    """The N(0, 1) draws of rng.h normals4 (one counter per sample and channel quad, Box-Muller on two pairs) as float64 values of the
    same Philox bits, with the band of their fp32 evaluation: rad = sqrtf(-2 logf(u)) -- logf 2 ulp, halved by the root, + 2 ulp of
    sqrtf = 3 ulp -- times sincosf (2 ulp) and the product's own half ulp: 5.5 ulp of |z|.  u and the fp32 product 2 pi v are exact."""
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


def _setup(m, B, rows=1):
    from dposer_amd import _C
    eng = m._engine()
    flat = m.flat_params()
    packed = eng.packed(flat, with_backward=False, force=True)
    ws = eng.workspace(B, _C.WS_SHARED_T, rows, torch.device(DEV))
    return eng, flat, packed, ws, eng.freq(torch.device(DEV), m._fourier_W())


def _refs(kind, N, scale, fourier, t32, nd, fn):
    """fn(scalars, used_sigma) for each admissible sigma index: one, except under the continuous VE kind with the positional lookup, whose
    index trunc(sigma(t)) is decided by a powf.  There the two references take floor(sigma - band) and floor(sigma + band): by construction
    these are the same index -- and the two references the same numbers -- wherever the band of sigma(t) holds no integer, so taking the
    smaller ratio admits a second index exactly where sde_ref.ambiguous_index holds and nowhere else."""
    sig = load("g8_scalars")["sigmas_buffer"]
    s = S._col(S.scalars(kind, t32, N=N, table=_table(kind, N)), nd) if np.ndim(t32) else S.scalars(kind, t32, N=N, table=_table(kind, N))
    lab = s["label"]
    if not isinstance(lab, S.E) and np.ndim(lab):
        lab = lab[(Ellipsis,) + (None,) * nd]
    sides = (-1, 1) if (kind == "ve" and scale and not fourier) else (0,)
    return [fn(s, S.used_sigma(sig, lab, fourier, scale, side)) for side in sides]


def _judge(name, got, refs, t32=None):
    r = S.ratio_any(got, refs)
    w = float(r.max()) if r.size else 0.0
    _log_measured("band_ratio_" + name, w)
    where = np.unravel_index(int(np.argmax(r)), r.shape) if r.size else ()
    at = "" if t32 is None or not where else f" at t = {float(np.asarray(t32).reshape(-1)[where[0]])!r}"
    print(f"{name}: worst band ratio {w:.3f}{at} (index {where})")
    assert w <= 1.0, f"{name}: worst band ratio {w:.3f}{at}, element {where}"


def test_sigma_buffer_is_the_fixture():
    """The sigmas the references index are the model's own buffer, bit for bit."""
    m, _ = _model(63, True)
    assert m.sigmas.cpu().numpy().tobytes() == load("g8_scalars")["sigmas_buffer"].tobytes()


# ---- per-sample t: the network forward (k_out_model), the whole grid as the rows of one call -----------------------------------------
@pytest.mark.parametrize("D", [63, 126])
@pytest.mark.parametrize("kind,N,scale", CASES, ids=_ids(CASES))
def test_forward_divides_by_the_sigma_of_every_label(kind, N, scale, D):
    """Under the continuous VE kind the caller hands sigma(t) in: here the fp32 rounding of the float64 sigma(t), and the division is judged
    at exactly that label.  (The library's own sigma(t), k_ve_labels and sde_at, is judged through the labels of test_pf_rhs_* and
    through every shared-t sweep.)"""
    m, c = _model(D, scale)
    t32 = _times(N)
    lab = S.scalars(kind, t32, N=N, table=_table(kind, N))["label"]
    lab32 = lab.v.astype(np.float32) if isinstance(lab, S.E) else lab
    x = _dev(np.random.RandomState(1).standard_normal((len(t32), D)).astype(np.float32))
    with torch.no_grad():
        out = m(x, _dev(lab32)).cpu().numpy()
    refs = [S.out_model(c[None, :], S.used_sigma(load("g8_scalars")["sigmas_buffer"], lab32.astype(np.float64)[:, None], False, scale))]
    _judge(f"forward_{kind}_N{N}_{'scaled' if scale else 'raw'}_D{D}", out, refs, t32)


@pytest.mark.parametrize("kind", ["subvp", "vp", "ve"])
def test_forward_fourier_divides_by_the_label(kind):
    m, c = _model(63, True, "fourier")
    t32 = _times(1000)
    lab = S.scalars(kind, t32)["label"]
    labels = _dev(lab.v.astype(np.float32) if isinstance(lab, S.E) else lab)
    x = _dev(np.random.RandomState(1).standard_normal((len(t32), 63)).astype(np.float32))
    with torch.no_grad():
        out = m(x, labels).cpu().numpy()
    ref = S.out_model(c[None, :], S.E(labels.cpu().numpy().astype(np.float64)[:, None]))
    _judge(f"forward_fourier_{kind}", out, ref, t32)


# ---- per-sample t: the DSM training step (k_prep_train + k_dsm), the time values as the rows of one call ----------------------------
def _dsm_case(kind, scale, D, t32, name, embedding="positional", draw=None):
    """fused_dsm_grad behind the constant network: the loss, the gradient of post_dense.bias -- the column sums of dres -- and every
    gradient upstream of post_dense, which is dres W_post with W_post = 0: exactly zero.  (The gradient of post_dense.weight itself is
    dres^T h with the last hidden activations h, which are not zero; it is not a function of the scalars alone and is not judged.)
    Sum chains: sde_ref.dsm_chains, counted from k_dsm, k_sum_partials and reduce_job_body.
    `draw` = (seed, step): t and z are drawn in the kernel (Philox) and regenerated here with oracle/philox.py."""
    from dposer_amd.algorithms.advanced.losses import fused_dsm_grad
    from oracle import philox as PH
    m, c = _model(D, scale, embedding)
    B = len(t32)
    rs = np.random.RandomState(1100 + B + D)
    x0 = rs.standard_normal((B, D)).astype(np.float32)
    if draw is None:
        z = rs.standard_normal((B, D)).astype(np.float32)
        kw = dict(t=_dev(t32), z=_dev(z), seed=3, step=0)
    else:
        t32 = np.asarray(PH.uniform_t(B, draw[1], draw[0]), np.float32)
        z = _drawn_normals(B, D, PH.STREAM_TRAIN_Z, draw[1], draw[0])
        kw = dict(seed=draw[0], step=draw[1])
    fg = torch.zeros(m._num_flat, device=DEV)
    loss = fused_dsm_grad(m, _sde(kind, 1000), _dev(x0), flat_grad=fg, **kw)
    loss, fg = loss.cpu().numpy(), fg.cpu().numpy()
    fourier = embedding == "fourier"
    refs = _refs(kind, 1000, scale, fourier, t32, 1, lambda s, us: S.dsm(kind, s, us, c[None, :], z))
    _judge(f"{name}_loss", loss, [r["loss"] for r in refs])
    seen = set()
    for (pname, prm), off in zip(m.named_parameters(), m._offsets):
        g = fg[off:off + prm.numel()]
        if pname == "post_dense.bias":
            _judge(f"{name}_bias_grad", g, [r["bias_grad"] for r in refs])
        elif pname != "post_dense.weight":
            assert not g.any(), f"{name}: the gradient of {pname} is not exactly zero"
        seen.add(pname)
    assert {"post_dense.bias", "post_dense.weight"} <= seen


@pytest.mark.parametrize("D", [63, 126])
@pytest.mark.parametrize("kind,N,scale", CONT, ids=_ids(CONT))
def test_dsm_step_with_every_time_value_as_a_row(kind, N, scale, D):
    _dsm_case(kind, scale, D, _times(N), f"dsm_{kind}_{'scaled' if scale else 'raw'}_D{D}")


@pytest.mark.parametrize("B", [1, 5, 33])
@pytest.mark.parametrize("kind,N,scale", CONT, ids=_ids(CONT))
def test_dsm_step_small_batches(kind, N, scale, B):
    """One row, five and 33 rows (one block of k_dsm, fewer samples than sample lanes): time values spread over the whole list."""
    t32 = _times(N)
    _dsm_case(kind, scale, 126 if B == 1 else 63, t32[np.linspace(0, len(t32) - 1, B).astype(int)], f"dsm_{kind}_{'scaled' if scale else 'raw'}_B{B}")


@pytest.mark.parametrize("kind", ["subvp", "vp", "ve"])
def test_dsm_step_fourier(kind):
    _dsm_case(kind, True, 63, _times(1000, every=10), f"dsm_fourier_{kind}", embedding="fourier")


@pytest.mark.parametrize("kind,N,scale", CONT, ids=_ids(CONT))
def test_big_dsm_step(kind, N, scale):
    """k_dsm's grid-stride loop: 16 sample lanes per block at Cp = 64 and at most 1024 blocks, so past 16384 samples a thread walks two;
    B = 16400 (B D = 1033200), three t repeated over the rows; 1024 partials of the loss and 1024 partial rows of the column sums."""
    _dsm_case(kind, scale, 63, np.resize(BIG_T, 16400), f"big_dsm_{kind}_{'scaled' if scale else 'raw'}")


@pytest.mark.parametrize("kind,N,scale", [c_ for c_ in CONT if c_[2]], ids=_ids([c_ for c_ in CONT if c_[2]]))
def test_dsm_step_with_in_kernel_draws(kind, N, scale):
    """t = None, z = None: k_prep_train draws t (u01 (T - eps) + eps) and z (Box-Muller) from Philox; oracle/philox.py regenerates them.
    t is two rounded fp32 operations and is regenerated bit for bit; z carries the band of `_drawn_normals`."""
    _dsm_case(kind, scale, 63, np.zeros(33, np.float32), f"dsm_drawn_{kind}", draw=(99, 3))


# ---- shared t: one call per t -------------------------------------------------------------------------------------------------------
def _prior_sweep(kind, N, scale, B, D, t32, embedding="positional"):
    """dposer_prior_loss (k_perturb_shared + k_denoise) at every t: weighted and not, under both reductions (mean: 1 / (B D); sum over the batch: 1 / B)."""
    from dposer_amd import _C
    m, c = _model(D, scale, embedding)
    eng, flat, packed, ws, freq = _setup(m, B)
    desc = _desc(kind, N)
    x0, z = _data(B, D, 100 + B + D)[:2]
    xd, zd = _dev(x0), _dev(z)
    G = len(t32)
    for weighted, inv_n, tag in ((True, 1.0 / (B * D), "w_mean"), (False, 1.0 / B, "u_sum"), (True, 1.0 / B, "w_sum"), (False, 1.0 / (B * D), "u_mean")):
        hat, grad, loss = (torch.empty((G, B, D), device=DEV), torch.empty((G, B, D), device=DEV), torch.empty(G, device=DEV))
        for i, t in enumerate(t32):
            _C.check(eng.lib.dposer_prior_loss(eng.h, _C.ptr(flat), _C.ptr(packed), _C.ptr(ws), C.byref(desc), _C.ptr(xd), _C.ptr(zd), float(t),
                                               1 if weighted else 0, float(inv_n), _C.ptr(hat[i]), _C.ptr(grad[i]), _C.ptr(loss[i:]), 0, 0,
                                               _C.ptr(freq), _C.ptr(m.sigmas), B, _C.stream_ptr()), "dposer_prior_loss")
        refs = _refs(kind, N, scale, embedding == "fourier", t32, 2,
                     lambda s, us: S.denoise(kind, s, us, x0[None], z[None], c[None, None, :], weighted, float(np.float32(inv_n)), per_row=True))
        name = f"prior_{kind}_N{N}_{'scaled' if scale else 'raw'}_{embedding[:3]}_B{B}_D{D}_{tag}"
        for k, got in (("x0_hat", hat), ("grad", grad), ("loss", loss)):
            _judge(f"{name}_{k}", got.cpu().numpy(), [r[k] for r in refs], t32)


@pytest.mark.parametrize("kind,N,scale", CASES, ids=_ids(CASES))
def test_prior_loss_on_the_whole_grid(kind, N, scale):
    _prior_sweep(kind, N, scale, 5, 63, _times(N))


@pytest.mark.parametrize("B,D", [(1, 126), (33, 126), (33, 63)])
@pytest.mark.parametrize("kind,N,scale", CASES, ids=_ids(CASES))
def test_prior_loss_other_shapes(kind, N, scale, B, D):
    """One sample / a 2-element tail, and 33 rows: element indexing does not depend on t, so every 10th grid value (all the edge values)."""
    _prior_sweep(kind, N, scale, B, D, _times(N, every=10))


@pytest.mark.parametrize("kind", ["subvp", "vp", "ve"])
def test_prior_loss_fourier(kind):
    _prior_sweep(kind, 1000, True, 5, 63, _times(1000, every=10), embedding="fourier")


SHAPES = [(5, 63), (1, 126), (33, 126)]          # the whole grid at (5, 63); one row / 33 rows with the 2-element quad tail at every 10th t


@pytest.mark.parametrize("B,D", SHAPES)
@pytest.mark.parametrize("kind,N,scale", CONT, ids=_ids(CONT))
def test_red_diff_on_the_grid(kind, N, scale, B, D):
    from dposer_amd import _C
    m, c = _model(D, scale)
    eng, flat, packed, ws, freq = _setup(m, B)
    desc = _desc(kind, N)
    t32 = _times(N, every=1 if (B, D) == (5, 63) else 10)
    x0, z = _data(B, D, 200 + B)[:2]
    xd, zd = _dev(x0), _dev(z)
    G = len(t32)
    eps, grad, loss = torch.empty((G, B, D), device=DEV), torch.empty((G, B, D), device=DEV), torch.empty(G, device=DEV)
    for i, t in enumerate(t32):
        _C.check(eng.lib.dposer_prior_red_diff(eng.h, _C.ptr(flat), _C.ptr(packed), _C.ptr(ws), C.byref(desc), _C.ptr(xd), _C.ptr(zd), float(t),
                                               1.0 / B, _C.ptr(eps[i]), _C.ptr(grad[i]), _C.ptr(loss[i:]), 0, 0, _C.ptr(freq), _C.ptr(m.sigmas),
                                               B, _C.stream_ptr()), "dposer_prior_red_diff")
    refs = _refs(kind, N, scale, False, t32, 2, lambda s, us: S.red_diff(kind, s, us, x0[None], z[None], c[None, None, :], per_row=True,
                                                                          inv_batch=1.0 / B))
    name = f"red_{kind}_{'scaled' if scale else 'raw'}_B{B}_D{D}"
    for k, got in (("eps_pred", eps), ("grad", grad), ("loss", loss)):
        _judge(f"{name}_{k}", got.cpu().numpy(), [r[k] for r in refs], t32)


@pytest.mark.parametrize("kind", ["ve_discrete", "vp_discrete"])
def test_discrete_kinds_are_refused_where_the_library_has_no_discrete_path(kind):
    """RED-Diff, the multi-step prior loss (scorefc.hip sde_kind_continuous) and the probability-flow right-hand side take the continuous
    score functions only: the C entries refuse a discrete descriptor and launch nothing, and prior.py routes such calls to the step-by-step
    compositions.  So these three are swept over the three continuous kinds; every other shared-t entry is swept over all five."""
    from dposer_amd import _C
    from dposer_amd.prior import _fused_variant_desc
    B, D, S_ = 5, 63, -777.0
    m, c = _model(D, True)
    eng, flat, packed, ws, freq = _setup(m, B, 2)
    desc = _desc(kind, 1000)
    assert _fused_variant_desc(m, _sde(kind, 1000), False) is None
    x0 = torch.zeros(B, D, device=DEV)
    outs = [torch.full((B, D), S_, device=DEV), torch.full((B, D), S_, device=DEV), torch.full((1,), S_, device=DEV)]
    ts = (C.c_float * 3)(0.5, 0.3, 0.1)
    rc = eng.lib.dposer_prior_red_diff(eng.h, _C.ptr(flat), _C.ptr(packed), _C.ptr(ws), C.byref(desc), _C.ptr(x0), None, 0.5, 1.0 / B,
                                       _C.ptr(outs[0]), _C.ptr(outs[1]), _C.ptr(outs[2]), 0, 0, _C.ptr(freq), _C.ptr(m.sigmas), B, _C.stream_ptr())
    assert rc != 0
    rc = eng.lib.dposer_prior_loss_multi(eng.h, _C.ptr(flat), _C.ptr(packed), _C.ptr(ws), C.byref(desc), _C.ptr(x0), None, ts, 2, 1, 1.0,
                                         _C.ptr(outs[0]), _C.ptr(outs[1]), _C.ptr(outs[2]), 0, 0, _C.ptr(freq), _C.ptr(m.sigmas), B, _C.stream_ptr())
    assert rc != 0
    state = torch.zeros(B * D + B, dtype=torch.float64, device=DEV)
    lab = torch.full((B,), S_, device=DEV)
    rc = _C.lib().dposer_pf_ode_rhs_begin(C.byref(desc), 0.5, _C.ptr(state), None, _C.ptr(outs[0]), _C.ptr(lab), None, B, D, _C.stream_ptr())
    assert rc != 0
    torch.cuda.synchronize()
    assert all(bool((o == S_).all()) for o in outs) and bool((lab == S_).all())


def _em_sweep(kind, N, scale, B, D, t32, completion):
    """dposer_em_sampler_steps, one step from a fresh x with injected noise: plain, or with observation and mask (imputation at t ahead of
    the predictor, sampling.py:459, and after it, :416-420; mask entries 0, 1, 0.25 and 0.625)."""
    from dposer_amd import _C
    m, c = _model(D, scale)
    eng, flat, packed, ws, freq = _setup(m, B)
    desc = _desc(kind, N)
    x, z, obs, zb = _data(B, D, 300 + B)
    za = _data(B, D, 301 + B)[0]
    mask = np.random.RandomState(302).choice(np.asarray([0.0, 1.0, 0.25, 0.625], np.float32), size=(B, D))
    G = len(t32)
    xs = _dev(np.broadcast_to(x, (G, B, D)).copy())
    means = torch.empty((G, B, D), device=DEV)
    noise = _dev(np.stack([za, z, zb]) if completion else z[None])
    obs_d, mask_d = (_dev(obs), _dev(mask)) if completion else (None, None)
    ts = np.ascontiguousarray(t32, dtype=np.float32)
    for i in range(G):
        _C.check(eng.lib.dposer_em_sampler_steps(eng.h, _C.ptr(flat), _C.ptr(packed), _C.ptr(ws), C.byref(desc), _C.ptr(xs[i]), _C.ptr(means[i]),
                                                 C.c_void_p(ts.ctypes.data + 4 * i), 0, 1, _C.ptr(obs_d), _C.ptr(mask_d), _C.ptr(noise), 0, None, 1,
                                                 _C.ptr(freq), _C.ptr(m.sigmas), B, _C.stream_ptr()), "dposer_em_sampler_steps")

    def ref(s, us):
        x_in = S.E(x[None])
        if completion:
            mk = S.E(mask[None])
            x_in = x_in * (1.0 - mk) + (s["mc"] * S.E(obs[None]) + S.E(za[None]) * s["sd"]) * mk
        return S.em_update(kind, s, None, us, x_in, c[None, None, :], z[None], N=N, obs=obs[None] if completion else None,
                           mask=mask[None] if completion else None, z_imp_b=zb[None] if completion else None)

    refs = _refs(kind, N, scale, False, t32, 2, ref)
    name = f"em_{'completion' if completion else 'plain'}_{kind}_N{N}_{'scaled' if scale else 'raw'}_B{B}_D{D}"
    _judge(f"{name}_x_mean", means.cpu().numpy(), [r["x_mean"] for r in refs], t32)
    _judge(f"{name}_x", xs.cpu().numpy(), [r["x"] for r in refs], t32)


@pytest.mark.parametrize("completion", [False, True], ids=["plain", "completion"])
@pytest.mark.parametrize("kind,N,scale", CASES, ids=_ids(CASES))
def test_em_step_on_the_whole_grid(kind, N, scale, completion):
    """Where the discrete-VP table shows: the drift g^2 score dt meets no std of marginal_prob (whose own fp32 cancellation at small t
    is wider than the table's former 4.3e-5).  Measured on the MI355X against a library built with the former fp32-running-product
    table: this sweep left the band by a factor 23.8 at t = 0.00401 (table index 4; vp_discrete, N = 1000, without scale_by_sigma) and
    55.8 at N = 2000 (t = 0.00200, index 4); the fused probability-flow step by 23.0 / 52.5, the Langevin norm sum by 10.1 / 23.5; all
    24 failing cases were discrete VP, every other case passed.  The float64 reference with that table in place of the fixture's predicts
    the same 23.8 (test_sde_ref_cpu.py::test_mutation_fp32_running_product_table); the host program of that file measured the header's
    table at 605 ulp there before the product was accumulated in double, 1 ulp since."""
    _em_sweep(kind, N, scale, 5, 63, _times(N), completion)


@pytest.mark.parametrize("kind,N,scale", [c_ for c_ in CASES if not c_[2]], ids=_ids([c_ for c_ in CASES if not c_[2]]))
def test_em_step_other_shapes(kind, N, scale):
    _em_sweep(kind, N, scale, 1, 126, _times(N, every=10), False)
    _em_sweep(kind, N, scale, 33, 126, _times(N, every=10), True)


@pytest.mark.parametrize("sampler", ["em_completion", "pf"])
@pytest.mark.parametrize("kind,N,scale", CASES, ids=_ids(CASES))
def test_whole_sampler_run_teacher_forced(kind, N, scale, sampler):
    """dposer_em_sampler with observation and mask, and dposer_pf_sampler, all N steps on linspace(T, 1e-5, N) with a trajectory buffer
    (the launch path: a trajectory keeps the call off the fused form, which test_fused_pf_step_* covers).  The reference recomputes step
    i from the kernel's own state after step i - 1, so nothing accumulates.  With an observation the recorded state of step i - 1 is the
    one BEFORE the look-ahead imputation, which the kernel of step i - 1 forms with the scalars at t_i (its t_next).  The mask holds 0, 1
    and the fractions 0.25 and 0.625: where it is 1 the imputation after the predictor overwrites whatever the look-ahead left, so only a
    fractional entry carries the look-ahead of step i - 1 into the recorded state of step i -- there a kernel that took the t_next
    scalars at t_{i-1} leaves the band at every step; the 0 / 1 entries see it in x_mean of the last step alone."""
    from dposer_amd import _C
    B, D = 5, 63
    m, c = _model(D, scale)
    eng, flat, packed, ws, freq = _setup(m, B, N)
    desc = _desc(kind, N)
    completion = sampler == "em_completion"
    t32 = torch.linspace(1.0, 1e-5, N).numpy()
    rs = np.random.RandomState(900)
    x0 = rs.standard_normal((B, D)).astype(np.float32)
    k_noise = 3 if completion else 1
    noise = rs.standard_normal((N, k_noise, B, D)).astype(np.float32)
    obs = rs.standard_normal((B, D)).astype(np.float32)
    mask = rs.choice(np.asarray([0.0, 1.0, 0.25, 0.625], np.float32), size=(B, D))
    x, x_mean, traj = _dev(x0), torch.empty((B, D), device=DEV), torch.empty((N, B, D), device=DEV)
    obs_d, mask_d = (_dev(obs), _dev(mask)) if completion else (None, None)
    fn = eng.lib.dposer_em_sampler if completion else eng.lib.dposer_pf_sampler
    ts = np.ascontiguousarray(t32)
    _C.check(fn(eng.h, _C.ptr(flat), _C.ptr(packed), _C.ptr(ws), C.byref(desc), _C.ptr(x), _C.ptr(x_mean), C.c_void_p(ts.ctypes.data), 0,
                _C.ptr(obs_d), _C.ptr(mask_d), _C.ptr(_dev(noise)), 0, _C.ptr(traj), 1, _C.ptr(freq), _C.ptr(m.sigmas), B, _C.stream_ptr()), sampler)
    got = traj.cpu().numpy()
    prev = np.concatenate([x0[None], got[:-1]])                     # the kernel's own state ahead of every step

    def ref(s, us):
        x_in = S.E(prev)
        if completion:
            mk = S.E(mask[None])
            x_in = x_in * (1.0 - mk) + (s["mc"] * S.E(obs[None]) + S.E(noise[:, 0]) * s["sd"]) * mk
            return S.em_update(kind, s, None, us, x_in, c[None, None, :], noise[:, 1], N=N, obs=obs[None], mask=mask[None], z_imp_b=noise[:, 2])
        return S.em_update(kind, s, None, us, x_in, c[None, None, :], None, N=N, pf=True)

    refs = _refs(kind, N, scale, False, t32, 2, ref)
    name = f"run_{sampler}_{kind}_N{N}_{'scaled' if scale else 'raw'}"
    _judge(f"{name}_traj", got, [r["x"] for r in refs], t32)
    _judge(f"{name}_x_mean_last", x_mean.cpu().numpy(), [r["x_mean"][-1] for r in refs])
    assert x.cpu().numpy().tobytes() == got[-1].tobytes()          # no look-ahead imputation after the last step


def _completion_sweep(kind, N, scale, B, D, t32):
    """dposer_completion_optimize, one Adam step (k_perturb_shared + k_completion_update) from given non-zero moments -- from zero moments
    Adam's first step is lr sign(g) whatever the scalars are.  Weighted at even positions of the time list, unweighted at odd ones."""
    from dposer_amd import _C
    m, c = _model(D, scale)
    eng, flat, packed, ws, freq = _setup(m, B)
    desc = _desc(kind, N)
    rs = np.random.RandomState(1000 + B)
    x0, z, obs = (rs.standard_normal((B, D)).astype(np.float32) for _ in range(3))
    mask = (rs.uniform(size=(B, D)) < 0.5).astype(np.float32)
    m0 = (1e-3 * rs.standard_normal((B, D))).astype(np.float32)
    v0 = (1e-6 * rs.uniform(0.5, 2.0, (B, D))).astype(np.float32)
    G = len(t32)
    lr, w_prior, w_data = 0.1, float(np.float32(0.7)), float(np.float32(1.3))
    xs, ms, vs = (_dev(np.broadcast_to(a, (G, B, D)).copy()) for a in (x0, m0, v0))
    zd, od, kd = _dev(z), _dev(obs), _dev(mask)
    for i, t in enumerate(t32):
        _C.check(eng.lib.dposer_completion_optimize(eng.h, _C.ptr(flat), _C.ptr(packed), _C.ptr(ws), C.byref(desc), _C.ptr(xs[i]), _C.ptr(od), _C.ptr(kd),
                                                    _C.ptr(ms[i]), _C.ptr(vs[i]), (C.c_float * 1)(float(t)), (C.c_int32 * 1)(1 - i % 2),
                                                    (C.c_float * 1)(w_prior), (C.c_float * 1)(w_data), 1, lr, 0.9, 0.999, 1e-8, _C.ptr(zd), 0, 0,
                                                    _C.ptr(freq), _C.ptr(m.sigmas), B, _C.stream_ptr()), "dposer_completion_optimize")
    got = dict(x=xs.cpu().numpy(), m=ms.cpu().numpy(), v=vs.cpu().numpy())
    for par in (0, 1):
        sel = np.arange(G)[par::2]
        refs = _refs(kind, N, scale, False, t32[sel], 2, lambda s, us: S.completion_update(
            kind, s, us, x0[None], z[None], c[None, None, :], obs[None], mask[None], m0[None], v0[None], par == 0, w_prior, w_data, lr, 0.9, 0.999, 1e-8))
        name = f"completion_{kind}_N{N}_{'scaled' if scale else 'raw'}_B{B}_D{D}_{'w' if par == 0 else 'u'}"
        for k in ("x", "m", "v"):
            _judge(f"{name}_{k}", got[k][sel], [r[k] for r in refs], t32[sel])


@pytest.mark.parametrize("B,D", [(5, 63), (1, 126), (33, 126)])
@pytest.mark.parametrize("kind,N,scale", CASES, ids=_ids(CASES))
def test_completion_adam_step_every_10th_t(kind, N, scale, B, D):
    _completion_sweep(kind, N, scale, B, D, _times(N, every=10))


def _pf_step_sweep(kind, N, scale, B, D, t32):
    """dposer_pf_sampler from start_step = N - 1: ONE probability-flow step.  Without observation and trajectory this is the fused form --
    post_dense and the Euler-Maruyama update in the GEMM epilogue (EpiEmStep, post_em_step), which carries its own copy of the
    update.  The time table is laid out so that its entry N - 1 is the t under test."""
    from dposer_amd import _C
    m, c = _model(D, scale)
    eng, flat, packed, ws, freq = _setup(m, B)
    desc = _desc(kind, N)
    x = _data(B, D, 800 + B)[0]
    G = len(t32)
    xs, means = _dev(np.broadcast_to(x, (G, B, D)).copy()), torch.empty((G, B, D), device=DEV)
    ts = np.ascontiguousarray(np.concatenate([np.ones(N - 1, np.float32), np.asarray(t32, np.float32)]))
    for i in range(G):
        _C.check(eng.lib.dposer_pf_sampler(eng.h, _C.ptr(flat), _C.ptr(packed), _C.ptr(ws), C.byref(desc), _C.ptr(xs[i]), _C.ptr(means[i]),
                                           C.c_void_p(ts.ctypes.data + 4 * i), N - 1, None, None, None, 0, None, 1, _C.ptr(freq),
                                           _C.ptr(m.sigmas), B, _C.stream_ptr()), "dposer_pf_sampler")
    refs = _refs(kind, N, scale, False, t32, 2, lambda s, us: S.em_update(kind, s, None, us, x[None], c[None, None, :], None, N=N, pf=True))
    name = f"pf_step_{kind}_N{N}_{'scaled' if scale else 'raw'}_B{B}_D{D}"
    _judge(f"{name}_x_mean", means.cpu().numpy(), [r["x_mean"] for r in refs], t32)
    _judge(f"{name}_x", xs.cpu().numpy(), [r["x"] for r in refs], t32)


@pytest.mark.parametrize("kind,N,scale", CASES, ids=_ids(CASES))
def test_fused_pf_step_on_the_whole_grid(kind, N, scale):
    _pf_step_sweep(kind, N, scale, 5, 63, _times(N))


@pytest.mark.parametrize("kind,N,scale", [c_ for c_ in CASES if not c_[2]], ids=_ids([c_ for c_ in CASES if not c_[2]]))
def test_fused_pf_step_other_shapes(kind, N, scale):
    _pf_step_sweep(kind, N, scale, 1, 126, _times(N, every=10))
    _pf_step_sweep(kind, N, scale, 33, 126, _times(N, every=10))


# ---- in-kernel noise -----------------------------------------------------------------------------------------------------------------
def _em_drawn_case(kind, N, scale, B, D, with_traj):
    """dposer_em_sampler_steps with noise = None, ONE step at each of three t (start_step = 0, 1, 2 of a three-entry time list, so the
    Philox offset of the draw is the step index): x_mean, which holds no draw, and x = x_mean + g sqrt(dt) z with z regenerated from
    oracle/philox.py (`_drawn_normals`, STREAM_EM_NOISE).  Without a trajectory buffer this is the fused form, the draw made in the GEMM
    epilogue; with one, k_em_update draws."""
    from dposer_amd import _C
    from oracle import philox as PH
    m, c = _model(D, scale)
    eng, flat, packed, ws, freq = _setup(m, B)
    desc = _desc(kind, N)
    x = _data(B, D, 1200 + B)[0]
    seed = 77
    ts = np.ascontiguousarray(BIG_T)
    G = len(ts)
    xs, means, traj = _dev(np.broadcast_to(x, (G, B, D)).copy()), torch.empty((G, B, D), device=DEV), torch.empty((G, B, D), device=DEV)
    for i in range(G):
        _C.check(eng.lib.dposer_em_sampler_steps(eng.h, _C.ptr(flat), _C.ptr(packed), _C.ptr(ws), C.byref(desc), _C.ptr(xs[i]), _C.ptr(means[i]),
                                                 C.c_void_p(ts.ctypes.data), i, 1, None, None, None, seed, _C.ptr(traj[i]) if with_traj else None, 1,
                                                 _C.ptr(freq), _C.ptr(m.sigmas), B, _C.stream_ptr()), "dposer_em_sampler_steps")
    zs = [_drawn_normals(B, D, PH.STREAM_EM_NOISE, i, seed) for i in range(G)]
    z = S.E(np.stack([a.v for a in zs]), np.stack([a.e for a in zs]))
    refs = _refs(kind, N, scale, False, ts, 2, lambda s, us: S.em_update(kind, s, None, us, x[None], c[None, None, :], z, N=N))
    name = f"em_drawn_{'launch' if with_traj else 'fused'}_{kind}_N{N}_{'scaled' if scale else 'raw'}_B{B}_D{D}"
    _judge(f"{name}_x_mean", means.cpu().numpy(), [r["x_mean"] for r in refs], ts)
    _judge(f"{name}_x", xs.cpu().numpy(), [r["x"] for r in refs], ts)
    if with_traj:
        assert traj.cpu().numpy().tobytes() == xs.cpu().numpy().tobytes()


@pytest.mark.parametrize("with_traj", [False, True], ids=["fused", "launch"])
@pytest.mark.parametrize("kind,N,scale", CASES, ids=_ids(CASES))
def test_em_step_with_in_kernel_noise(kind, N, scale, with_traj):
    _em_drawn_case(kind, N, scale, 33, 63, with_traj)


# ---- shared t, every 10th t: the multi-step (DDIM) estimate --------------------------------------------------------------------------
@pytest.mark.parametrize("B,D", SHAPES)
@pytest.mark.parametrize("n_steps", [2, 5])
@pytest.mark.parametrize("kind,N,scale", CONT, ids=_ids(CONT))
def test_multi_step_prior_every_10th_t(kind, N, scale, n_steps, B, D):
    from dposer_amd.prior import multi_step_prior_eval, multi_step_time_grid
    m, c = _model(D, scale)
    sde = _sde(kind, N)
    t32 = _times(N, every=10)
    x0, z = _data(B, D, 400 + B)[:2]
    xd, zd = _dev(x0), _dev(z)
    G = len(t32)
    inv_n = 1.0 / (B * D)
    sig = load("g8_scalars")["sigmas_buffer"]
    for weighted in ((True, False) if (B, D) == (5, 63) else (True,)):          # the unweighted branch of the last k_ddim_step at one shape
        hat, grad, losses, trajs = torch.empty((G, B, D), device=DEV), torch.empty((G, B, D), device=DEV), [], []
        for i, t in enumerate(t32):
            trajs.append(multi_step_time_grid(float(t), n_steps))
            loss, _, _ = multi_step_prior_eval(m, sde, xd, trajs[-1], weighted=weighted, inv_n=inv_n, z=zd, x0_hat=hat[i], grad=grad[i])
            losses.append(loss)
        traj = np.asarray(trajs, dtype=np.float32)                      # [G, n + 1]
        refs = []
        for side in ((-1, 1) if (kind == "ve" and scale) else (0,)):
            ss = [S._col(S.scalars(kind, traj[:, j], N=N), 2) for j in range(n_steps + 1)]
            us = [S.used_sigma(sig, s["label"] if isinstance(s["label"], S.E) else s["label"][:, None, None], False, scale, side) for s in ss]
            refs.append(S.ddim(kind, ss, us, x0[None], z[None], c[None, None, :], weighted, float(np.float32(inv_n)), per_row=True))
        name = f"multi{n_steps}_{kind}_{'scaled' if scale else 'raw'}_B{B}_D{D}_{'w' if weighted else 'u'}"
        _judge(f"{name}_x0_hat", hat.cpu().numpy(), [r["x0_hat"] for r in refs], t32)
        _judge(f"{name}_grad", grad.cpu().numpy(), [r["grad"] for r in refs], t32)
        _judge(f"{name}_loss", torch.cat(losses).cpu().numpy(), [r["loss"] for r in refs], t32)


@pytest.mark.parametrize("B,D", [(33, 63), (1, 126), (5, 126)])
@pytest.mark.parametrize("kind,N,scale", CASES, ids=_ids(CASES))
def test_langevin_step_every_10th_t(kind, N, scale, B, D):
    """dposer_langevin_step, both phases: the two norm sums of phase 0, x_mean and x of phase 1 (which reads the kernel's own sums; the
    reference carries the band of its float64 sums through the step size).  The score here meets no marginal std either, so an error
    of the discrete-VP table reaches the norm sum of the scores undiminished."""
    from dposer_amd import _C
    m, c = _model(D, scale)
    eng, flat, packed, ws, freq = _setup(m, B)
    desc = _desc(kind, N)
    t32 = _times(N, every=10)
    x, nz = _data(B, D, 700 + B)[:2]
    G = len(t32)
    snr, alpha = float(np.float32(0.16)), float(np.float32(0.97))
    xs, means, sums = _dev(np.broadcast_to(x, (G, B, D)).copy()), torch.empty((G, B, D), device=DEV), torch.empty((G, 2), device=DEV)
    nd = _dev(nz)
    for i, t in enumerate(t32):
        for phase in (0, 1):
            _C.check(eng.lib.dposer_langevin_step(eng.h, _C.ptr(flat), _C.ptr(packed), _C.ptr(ws), C.byref(desc), _C.ptr(xs[i]), _C.ptr(means[i]),
                                                  float(t), alpha, snr, _C.ptr(nd), 0, 0, _C.ptr(sums[i]), phase, 1.0 / B, _C.ptr(freq),
                                                  _C.ptr(m.sigmas), B, _C.stream_ptr()), "dposer_langevin_step")
    cc = np.broadcast_to(c, (B, D))[None]
    refs = _refs(kind, N, scale, False, t32, 2, lambda s, us: S.langevin(kind, s, us, x[None], cc, np.broadcast_to(nz, (G, B, D)), snr, alpha))
    name = f"langevin_{kind}_N{N}_{'scaled' if scale else 'raw'}_B{B}_D{D}"
    got = sums.cpu().numpy()
    _judge(f"{name}_grad_norm_sum", got[:, 0], [r["gsum"] for r in refs], t32)
    _judge(f"{name}_noise_norm_sum", got[:, 1], [r["nsum"] for r in refs], t32)
    _judge(f"{name}_x_mean", means.cpu().numpy(), [r["x_mean"] for r in refs], t32)
    _judge(f"{name}_x", xs.cpu().numpy(), [r["x"] for r in refs], t32)


# ---- no network: the probability-flow ODE right-hand side ------------------------------------------------------------------------------
@pytest.mark.parametrize("B,D", [(5, 63), (1, 126), (33, 126)])
@pytest.mark.parametrize("kind", ["subvp", "vp", "ve"])
def test_pf_rhs_on_the_whole_grid(kind, B, D):
    from dposer_amd import _C
    lib = _C.lib()
    desc = _desc(kind, 1000)
    t32 = _times(1000) if B == 5 else _times(1000, every=10)
    x, noise, out, dx = _data(B, D, 500 + B)
    G = len(t32)
    state = _dev(np.concatenate([x.reshape(-1).astype(np.float64), np.zeros(B)]))
    nz, od, dxd = _dev(noise), _dev(out), _dev(dx)
    xf, labels = torch.empty((G, B, D), device=DEV), torch.empty((G, B), device=DEV)
    dout = torch.empty((G, B, D), device=DEV)
    dstate = torch.empty((G, B * D + B), dtype=torch.float64, device=DEV)
    drift_only = torch.empty((G, B * D), dtype=torch.float64, device=DEV)
    st = _C.stream_ptr()
    for i, t in enumerate(t32):
        _C.check(lib.dposer_pf_ode_rhs_begin(C.byref(desc), float(t), _C.ptr(state), _C.ptr(nz), _C.ptr(xf[i]), _C.ptr(labels[i]), _C.ptr(dout[i]), B, D, st),
                 "dposer_pf_ode_rhs_begin")
        _C.check(lib.dposer_pf_ode_rhs_end(C.byref(desc), float(t), _C.ptr(xf[i]), _C.ptr(od), _C.ptr(dxd), _C.ptr(nz), _C.ptr(dstate[i]), B, D, st),
                 "dposer_pf_ode_rhs_end")
        _C.check(lib.dposer_pf_ode_rhs_end(C.byref(desc), float(t), _C.ptr(xf[i]), _C.ptr(od), None, None, _C.ptr(drift_only[i]), B, D, st),
                 "dposer_pf_ode_rhs_end")
    s = S._col(S.scalars(kind, t32), 2)
    ref = S.pf_rhs(kind, s, x[None], out[None], noise[None], dx[None])
    assert xf.cpu().numpy().tobytes() == np.broadcast_to(x, (G, B, D)).astype(np.float32).tobytes()
    lab = S.scalars(kind, t32)["label"]
    if isinstance(lab, S.E):
        _judge(f"pf_{kind}_labels", labels.cpu().numpy(), lab[:, None], t32)
    else:
        assert labels.cpu().numpy().tobytes() == np.broadcast_to(lab[:, None], (G, B)).astype(np.float32).tobytes()      # exact
    ds = dstate.cpu().numpy()
    name = f"pf_{kind}_B{B}_D{D}"
    _judge(f"{name}_dout", dout.cpu().numpy(), ref["dout"], t32)
    _judge(f"{name}_drift", ds[:, :B * D].reshape(G, B, D), ref["drift"], t32)
    _judge(f"{name}_hutchinson", ds[:, B * D:], ref["hutch"], t32)
    assert drift_only.cpu().numpy().tobytes() == ds[:, :B * D].tobytes()


# ---- the grid-stride loops and the partial sums: one case per reducing kernel just above 256 x 1024, three t -----------------------------
BIG_T = np.asarray([1.0, 0.5005005, 1e-3], np.float32)


@pytest.mark.parametrize("kind,N,scale", CASES, ids=_ids(CASES))
def test_big_prior_loss(kind, N, scale):
    """k_denoise + k_sum_partials: B D = 262269 > 256 x 1024, so the first threads make two passes and 1024 partials are summed."""
    from dposer_amd import _C
    D, B = 63, 4163
    m, c = _model(D, scale)
    eng, flat, packed, ws, freq = _setup(m, B)
    desc = _desc(kind, N)
    x0, z = _data(B, D, 600)[:2]
    xd, zd = _dev(x0), _dev(z)
    inv_n = 1.0 / (B * D)
    for t in BIG_T:
        hat, grad, loss = torch.empty((B, D), device=DEV), torch.empty((B, D), device=DEV), torch.empty(1, device=DEV)
        _C.check(eng.lib.dposer_prior_loss(eng.h, _C.ptr(flat), _C.ptr(packed), _C.ptr(ws), C.byref(desc), _C.ptr(xd), _C.ptr(zd), float(t), 1,
                                           float(inv_n), _C.ptr(hat), _C.ptr(grad), _C.ptr(loss), 0, 0, _C.ptr(freq), _C.ptr(m.sigmas), B,
                                           _C.stream_ptr()), "dposer_prior_loss")
        refs = _refs(kind, N, scale, False, t, 0, lambda s, us: S.denoise(kind, s, us, x0, z, c[None, :], True, float(np.float32(inv_n))))
        for k, got in (("x0_hat", hat), ("grad", grad), ("loss", loss[0])):
            _judge(f"big_prior_{kind}_N{N}_{'scaled' if scale else 'raw'}_{k}", got.cpu().numpy(), [r[k] for r in refs])


@pytest.mark.parametrize("kind,N,scale", CONT, ids=_ids(CONT))
def test_big_red_diff_and_ddim(kind, N, scale):
    """k_red_diff and the last k_ddim_step walk quads: B ceil(D / 4) = 262160 > 256 x 1024 at B = 16385 (two passes, four terms each)."""
    from dposer_amd import _C
    from dposer_amd.prior import multi_step_prior_eval, multi_step_time_grid
    D, B = 63, 16385
    m, c = _model(D, scale)
    eng, flat, packed, ws, freq = _setup(m, B, 2)
    desc = _desc(kind, N)
    x0, z = _data(B, D, 601)[:2]
    xd, zd = _dev(x0), _dev(z)
    sig = load("g8_scalars")["sigmas_buffer"]
    tag = f"{kind}_{'scaled' if scale else 'raw'}"
    for t in BIG_T:
        eps, rgrad, rloss = torch.empty((B, D), device=DEV), torch.empty((B, D), device=DEV), torch.empty(1, device=DEV)
        _C.check(eng.lib.dposer_prior_red_diff(eng.h, _C.ptr(flat), _C.ptr(packed), _C.ptr(ws), C.byref(desc), _C.ptr(xd), _C.ptr(zd), float(t),
                                               1.0 / B, _C.ptr(eps), _C.ptr(rgrad), _C.ptr(rloss), 0, 0, _C.ptr(freq), _C.ptr(m.sigmas), B,
                                               _C.stream_ptr()), "dposer_prior_red_diff")
        refs = _refs(kind, N, scale, False, t, 0, lambda s, us: S.red_diff(kind, s, us, x0, z, c[None, :]))
        for k, got in (("eps_pred", eps), ("grad", rgrad), ("loss", rloss[0])):
            _judge(f"big_red_{tag}_{k}", got.cpu().numpy(), [r[k] for r in refs])
        traj = multi_step_time_grid(float(t), 2)
        inv_n = 1.0 / (B * D)
        loss, grad, hat = multi_step_prior_eval(m, _sde(kind, N), xd, traj, weighted=True, inv_n=inv_n, z=zd)
        refs = []
        for side in ((-1, 1) if (kind == "ve" and scale) else (0,)):
            ss = [S.scalars(kind, np.float32(v), N=N) for v in traj]
            us = [S.used_sigma(sig, s_["label"], False, scale, side) for s_ in ss]
            refs.append(S.ddim(kind, ss, us, x0, z, c[None, :], True, float(np.float32(inv_n))))
        for k, got in (("x0_hat", hat), ("grad", grad), ("loss", loss[0])):
            _judge(f"big_multi2_{tag}_{k}", got.cpu().numpy(), [r[k] for r in refs])


@pytest.mark.parametrize("kind,N,scale", CASES, ids=_ids(CASES))
def test_big_langevin(kind, N, scale):
    """k_langevin_norms + k_sum_partials2 at B D just above 256 x 1024 (B = 4163: 17 blocks of partials for each of the two sums)."""
    from dposer_amd import _C
    D, B = 63, 4163
    m, c = _model(D, scale)
    eng, flat, packed, ws, freq = _setup(m, B)
    desc = _desc(kind, N)
    x, nz = _data(B, D, 602)[:2]
    snr, alpha = float(np.float32(0.16)), float(np.float32(0.97))
    nd = _dev(nz)
    cc = np.broadcast_to(c, (B, D))
    for t in BIG_T:
        xs, means, sums = _dev(x), torch.empty((B, D), device=DEV), torch.empty(2, device=DEV)
        for phase in (0, 1):
            _C.check(eng.lib.dposer_langevin_step(eng.h, _C.ptr(flat), _C.ptr(packed), _C.ptr(ws), C.byref(desc), _C.ptr(xs), _C.ptr(means), float(t),
                                                  alpha, snr, _C.ptr(nd), 0, 0, _C.ptr(sums), phase, 1.0 / B, _C.ptr(freq), _C.ptr(m.sigmas), B,
                                                  _C.stream_ptr()), "dposer_langevin_step")
        refs = _refs(kind, N, scale, False, t, 0, lambda s, us: S.langevin(kind, s, us, x, cc, nz, snr, alpha))
        name = f"big_langevin_{kind}_N{N}_{'scaled' if scale else 'raw'}"
        got = sums.cpu().numpy()
        _judge(f"{name}_grad_norm_sum", got[0], [r["gsum"] for r in refs])
        _judge(f"{name}_noise_norm_sum", got[1], [r["nsum"] for r in refs])
        _judge(f"{name}_x_mean", means.cpu().numpy(), [r["x_mean"] for r in refs])
        _judge(f"{name}_x", xs.cpu().numpy(), [r["x"] for r in refs])


@pytest.mark.parametrize("kind", ["subvp", "vp", "ve"])
def test_big_pf_rhs(kind):
    """k_pf_rhs_begin's grid-stride loop (B D = 262269 elements) and k_pf_rhs_end's 1041 blocks of four rows."""
    from dposer_amd import _C
    lib = _C.lib()
    D, B = 63, 4163
    desc = _desc(kind, 1000)
    x, noise, out, dx = _data(B, D, 603)
    state = _dev(np.concatenate([x.reshape(-1).astype(np.float64), np.zeros(B)]))
    nz, od, dxd = _dev(noise), _dev(out), _dev(dx)
    st = _C.stream_ptr()
    for t in BIG_T:
        xf, labels, dout = torch.empty((B, D), device=DEV), torch.empty(B, device=DEV), torch.empty((B, D), device=DEV)
        dstate = torch.empty(B * D + B, dtype=torch.float64, device=DEV)
        _C.check(lib.dposer_pf_ode_rhs_begin(C.byref(desc), float(t), _C.ptr(state), _C.ptr(nz), _C.ptr(xf), _C.ptr(labels), _C.ptr(dout), B, D, st),
                 "dposer_pf_ode_rhs_begin")
        _C.check(lib.dposer_pf_ode_rhs_end(C.byref(desc), float(t), _C.ptr(xf), _C.ptr(od), _C.ptr(dxd), _C.ptr(nz), _C.ptr(dstate), B, D, st),
                 "dposer_pf_ode_rhs_end")
        ref = S.pf_rhs(kind, S.scalars(kind, t), x, out, noise, dx)
        assert xf.cpu().numpy().tobytes() == x.tobytes()
        ds = dstate.cpu().numpy()
        _judge(f"big_pf_{kind}_dout", dout.cpu().numpy(), ref["dout"])
        _judge(f"big_pf_{kind}_drift", ds[:B * D].reshape(B, D), ref["drift"])
        _judge(f"big_pf_{kind}_hutchinson", ds[B * D:], ref["hutch"])
