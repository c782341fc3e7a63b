"""Every GEMM tiling of the score network against the float64 oracle, forced onto the smallest batch that can hold it.

The tiling follows the padded batch (csrc/scorefc.hip: 128x32 up to 2048 samples, 128x128 above, 256x256 from 16384; 64x32 / 64x128 for
post_dense and dx; the weight gradients and the time-branch dgrad change form as well), and an oracle cannot follow it there.  Here the
policies ``score_plan.POLICY_BIG`` (256x256 everywhere, 64x128, 256x256 weight gradients) and ``POLICY_MID`` (128x128 everywhere, 64x128)
are loaded through ``tuning_env`` and every case first asserts through ``dposer_scorefc_plan`` that they took.  Batches: one tile with
padding rows (BIG 200 -> 256, MID 65 -> 128), several tiles with the last real row alone in its tile (513 -> 768: three 256-row tiles,
or six 128-row tiles of which the sixth is all padding), and D = 126 (two 64-channel output blocks on the 64x128 tiling).

Reference: oracle/score_ref.py in float64 (parameters and inputs cast to double) with the Philox dropout masks of oracle/philox.py.
Whole-tensor bounds are the ones the 128x32 tiling is held to in tests/test_gpu_score.py (forward TOL_FP32, loss 5e-5, parameter
gradient 3e-4, x.grad 2e-4, sampler 1e-4, prior loss and gradient 2e-4).  Every 2-D gradient is also judged per aligned 32 x 32 tile
(``bf16_ref.tile_err``), so that a misplaced or half-summed tile cannot hide in the tensor norm: per tensor the bound is F times the
worst-tile error of the float32-arithmetic CPU oracle against the float64 one, F = 4 x R_max rounded up to a power of two, R_max the
largest measured ratio (GPU worst tile) / (float32 oracle worst tile) over all cases, the default policy included.

Measured on the MI355X (DPOSER_LOG_ERR), largest over all cases, bound beside it: forward 3.0e-6 fp32 / 8.4e-6 bf16x3 (2e-5); loss 1.2e-7 /
1.0e-6 (5e-5); parameter gradient 8.9e-6 / 1.5e-5 (3e-4); x.grad 4.0e-6 / 1.2e-5 (2e-4); sampler 2.6e-6 / 7.9e-6 (1e-4); prior loss 5.9e-7 /
1.7e-6 and its gradient 2.7e-6 / 7.9e-6 (2e-4).  Worst 32 x 32 tile of a gradient: 2.2e-5 / 2.7e-5 where the float32 oracle has 2.2e-5;
R_max = 1.16 in fp32 (b2_dense1.weight, MID at B = 65, dropout on) and 4.32 in bf16x3 (post_dense.weight, BIG at B = 513, no dropout;
per tensor 1.4 ... 4.3: three bf16 products and their fp32 sums stand in for one fp32 product), so F = 8 and F = 32.  The same inputs
give the same ratios under the default, MID and BIG policies to two digits: no tiling is further from float64 than 128x32 is.

The workspace handed to the library is the 256-byte-aligned middle of a larger allocation with 64 KiB of a byte pattern on either
side (``guards``): the slab, partial and aux capacities of the layout depend on the same policy functions, and the guards must be
intact after every call."""
import functools

import numpy as np
import pytest
import torch

import bf16_ref as Q
import score_plan as SP
from gpu_common import DEV, TOL_FP32, make_model, t2n
from helpers import _log_measured, rel_err
from oracle import philox as PH
from oracle import score_ref as R

pytestmark = pytest.mark.gpu
torch.set_num_threads(8)

# R_max (largest GPU worst-tile error over the float32 oracle's, all cases and tensors) and F = 4 x R_max rounded up to a power of two
TILE_R_MAX = {"fp32": 1.164, "bf16x3": 4.322}
TILE_FACTOR = {"fp32": 8.0, "bf16x3": 32.0}

WEIGHT_SEED, STEP_NODROP, STEP_DROP, DROP_P, SAMPLER_SEED = 61, 0, 7, 0.1, 17
CASES = [("BIG", 200, 63), ("BIG", 513, 63), ("BIG", 200, 126),
         ("MID", 65, 63), ("MID", 513, 63), ("MID", 200, 126),
         ("default", 65, 63), ("default", 200, 63), ("default", 513, 63), ("default", 200, 126)]
PRECS = ["fp32", "bf16x3"]


def _dev(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.float32).to(DEV)


# ------------------------------------------------------------------------------------------------
# guarded workspaces
# ------------------------------------------------------------------------------------------------
GUARD, PATTERN = 65536, 0xA5


class _Guards:
    def __init__(self):
        self.bufs = []

    def alloc(self, need, device):
        raw = torch.full((need + 2 * GUARD + 256,), PATTERN, dtype=torch.uint8, device=device)
        off = GUARD + (-(raw.data_ptr() + GUARD)) % 256
        self.bufs.append((raw, off, need))
        return raw[off:off + need]

    def check(self):
        assert self.bufs, "no workspace was handed out through the guarded allocator"
        for raw, off, need in self.bufs:
            assert bool((raw[:off] == PATTERN).all()), "bytes in front of the workspace were written"
            assert bool((raw[off + need:] == PATTERN).all()), "bytes behind the workspace were written"


@pytest.fixture
def guards(monkeypatch):
    from dposer_amd import _C
    from dposer_amd.engine import ScoreEngine, TrainWorkspaceLease
    g = _Guards()

    def workspace(self, batch, mode, n_steps, device):
        need = self.lib.dposer_scorefc_workspace_bytes(self.h, batch, mode, n_steps)
        assert need > 0
        return g.alloc(need, device)

    def lease(self, batch, device):
        need = self.lib.dposer_scorefc_workspace_bytes(self.h, batch, _C.WS_TRAIN, 0)
        assert need > 0
        return TrainWorkspaceLease([], g.alloc(need, device))

    monkeypatch.setattr(ScoreEngine, "workspace", workspace)
    monkeypatch.setattr(ScoreEngine, "lease_train_workspace", lease)
    return g


# ------------------------------------------------------------------------------------------------
# the float64 (and, for the tile bounds, float32) oracle of a batch: computed once, shared, never modified
# ------------------------------------------------------------------------------------------------
def _params(D, dt):
    from weights import make_weights
    p = {k: v.to(dt) if v.is_floating_point() else v for k, v in make_weights(WEIGHT_SEED, D=D).items()}
    p["sigmas"] = R.sigma_table()
    return p


@functools.lru_cache(maxsize=None)
def _inputs(B, D):
    rs = np.random.RandomState(1000 * D + B)
    x = (rs.standard_normal((B, D)) * 0.5).astype(np.float32)
    t = rs.uniform(1e-3, 1.0, B).astype(np.float32)
    z = rs.standard_normal((B, D)).astype(np.float32)
    w = rs.standard_normal((B, D)).astype(np.float32)
    labels = (t * np.float32(999.0)).astype(np.float32)
    # the float64 oracle must look up the same row of the sigma table as the kernels, which form t * 999 in float32
    assert np.array_equal(np.floor(labels.astype(np.float64)), np.floor(t.astype(np.float64) * 999.0))
    return x, t, z, w, labels


def _grads(p, loss, names):
    gr = torch.autograd.grad(loss, [p[n] for n in names], allow_unused=True)
    return {n: (None if g is None else g.detach()) for n, g in zip(names, gr)}


@functools.lru_cache(maxsize=None)
def _dsm_ref(B, D, drop, rng_seed, dt):
    """(loss, {name: gradient}) of the DSM loss in arithmetic ``dt`` with the Philox masks of (rng_seed, STEP_DROP) when ``drop``."""
    x, t, z, _, _ = _inputs(B, D)
    names = R.param_names()
    p = _params(D, dt)
    for n in names:
        p[n] = p[n].clone().requires_grad_(True)
    kw = {}
    if drop:
        kw = dict(drop_masks=_masks(B, rng_seed), drop_p=DROP_P)
    loss = R.dsm_loss(p, R.SubVP(), torch.tensor(x).to(dt), torch.tensor(t).to(dt), torch.tensor(z).to(dt), **kw)
    return loss.item(), _grads(p, loss, names)


@functools.lru_cache(maxsize=None)
def _masks(B, rng_seed):
    return tuple(torch.tensor(PH.dropout_keep_mask(B, 1024, site, STEP_DROP, rng_seed, DROP_P)) for site in range(5))


@functools.lru_cache(maxsize=None)
def _fwd_ref(B, D, dt):
    """Eval forward, and the gradient of sum(out * w) with respect to x, in arithmetic ``dt``."""
    x, _, _, w, labels = _inputs(B, D)
    xr = torch.tensor(x).to(dt).requires_grad_(True)
    out = R.scorefc_forward(_params(D, dt), xr, torch.tensor(labels).to(dt))
    dx, = torch.autograd.grad((out * torch.tensor(w).to(dt)).sum(), [xr])
    return out.detach(), dx.detach()


@functools.lru_cache(maxsize=None)
def _sampler_ref(B, D):
    _, _, z, _, _ = _inputs(B, D)
    noises = [torch.tensor(PH.normal_matrix(B, D, PH.STREAM_EM_NOISE, i, SAMPLER_SEED)).double() for i in range(3)]
    with torch.no_grad():
        return R.pc_sampler(_params(D, torch.float64), R.SubVP(N=3), torch.tensor(z).double(), noises)[1]


@functools.lru_cache(maxsize=None)
def _prior_ref(B, D, tt, weighted):
    x, _, z, _, _ = _inputs(B, D)
    with torch.no_grad():
        l, g = R.dposer_prior_loss(_params(D, torch.float64), R.SubVP(), torch.tensor(x).double(), torch.full((B,), tt, dtype=torch.float64),
                                   torch.tensor(z).double(), weighted=weighted)
    return float(l), g


# ------------------------------------------------------------------------------------------------
# policies and their plans
# ------------------------------------------------------------------------------------------------
def _expected_tiles(policy):
    if policy == "default":
        return (SP.SMALL, SP.SMALL, SP.SMALL, SP.FINAL_S, SP.MID)
    tile = SP.GEMM_OF[policy]
    return (tile, tile, tile, SP.FINAL, tile)


def _assert_plan(m, policy, B, prec, *, batched=True, events=False, silu_split_off=False):
    pl = SP.model_plan(m, B, events)
    padded = (B + 63) // 64 * 64 if B <= 512 else (B + 255) // 256 * 256
    assert (pl.padded, pl.gn, pl.gn_bwd, pl.time, pl.final, pl.wgrad) == (padded,) + _expected_tiles(policy), (policy, B, pl)
    lanes = prec != "fp32" and batched and not events                      # (fp32 reads transposed operand copies: split-K launches only)
    assert (pl.wgrad_form, pl.groups) == ((SP.ONE_LAUNCH, 0) if lanes else (SP.SPLIT_K, 0)), pl
    assert pl.time_split == (1 if prec == "bf16x3" else 0), pl              # (the k-split form of bf16 needs sample-major weight gradients)
    assert pl.side_stream == 0
    return pl


class _Checks:
    """Measure, log, and fail at the end of the case: one run then shows every figure of a case, not only the first that misses."""

    def __init__(self, tag):
        self.tag, self.failed = tag, []

    def bound(self, what, value, bound):
        _log_measured(what, value)
        if not value <= bound:
            self.failed.append(f"{what}: {value:.3e} > {bound:.3e}")

    def tiles(self, what, got, want64, want32, prec):
        """A 2-D gradient per aligned 32 x 32 tile: GPU against float64 within TILE_FACTOR x (float32 oracle against float64)."""
        e_gpu, e_ref = Q.tile_err(got, want64), Q.tile_err(want32, want64)
        _log_measured("tile_err/" + what, e_gpu)
        _log_measured("tile_ref/" + what, e_ref)
        _log_measured("tile_ratio/" + prec + "/" + what, e_gpu / e_ref)
        print(f"{self.tag} {what}: worst tile {e_gpu:.2e}, float32 oracle {e_ref:.2e}, ratio {e_gpu / e_ref:.2f}")
        if not e_gpu <= TILE_FACTOR[prec] * e_ref:
            self.failed.append(f"tile {what}: {e_gpu:.3e} > {TILE_FACTOR[prec]:.0f} x {e_ref:.3e}")

    def done(self):
        assert not self.failed, self.tag + "\n" + "\n".join(self.failed)


def _check_param_grads(ck, label, m, fg, B, D, drop, prec):
    _, g64 = _dsm_ref(B, D, drop, m._rng_seed, torch.float64)
    _, g32 = _dsm_ref(B, D, drop, m._rng_seed, torch.float32)
    for (name, prm), off in zip(m.named_parameters(), m._offsets):
        got = fg[off:off + prm.numel()].detach().double().cpu().reshape(prm.shape)
        if g64[name] is None:
            assert float(got.abs().max()) == 0.0, name                 # pre_dense_cond: exactly zero
            continue
        ck.bound(f"{label}/grad/{name}", float((got - g64[name]).norm() / g64[name].norm()), 3e-4)
        if got.dim() == 2:
            ck.tiles(f"{label}/{name}", got, g64[name], g32[name], prec)


# ------------------------------------------------------------------------------------------------
# the tests
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("policy,B,D", CASES)
def test_forward_and_autograd_vs_float64_oracle(policy, B, D, prec, tuning_env, guards):
    SP.force(tuning_env, policy)
    cfg, m, p = make_model(WEIGHT_SEED, D=D, precision=prec, dropout=DROP_P)
    _assert_plan(m, policy, B, prec)
    x, _, _, w, labels = _inputs(B, D)
    ck = _Checks(f"{policy} B={B} D={D} {prec}")
    out64, dx64 = _fwd_ref(B, D, torch.float64)
    _, dx32 = _fwd_ref(B, D, torch.float32)
    with torch.no_grad():
        out = m(_dev(x), _dev(labels))
    guards.check()
    ck.bound("forward", rel_err(t2n(out), out64.numpy()), TOL_FP32)
    xd = _dev(x).requires_grad_(True)
    out_a = m(xd, _dev(labels))
    (out_a * _dev(w)).sum().backward()
    guards.check()
    ck.bound("autograd/out", rel_err(t2n(out_a), out64.numpy()), TOL_FP32)
    ck.bound("autograd/x.grad", rel_err(t2n(xd.grad), dx64.numpy()), 2e-4)
    ck.tiles("autograd/x.grad", t2n(xd.grad), dx64, dx32, prec)
    ck.done()


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("policy,B,D", CASES)
def test_fused_dsm_step_vs_float64_oracle_with_philox_masks(policy, B, D, prec, tuning_env, guards):
    """Loss and every parameter gradient of the fused training step, without dropout and with the in-kernel Philox dropout against the
    restated masks (a wrong sample index in a tiling's training epilogue would still give self-consistent gradients); then the other
    forms of the weight gradients and of the time-branch dgrad under the same tiling, and the bucketed backward."""
    from dposer_amd.algorithms.advanced import sde_lib
    from dposer_amd.algorithms.advanced.losses import fused_dsm_grad
    SP.force(tuning_env, policy)
    x, t, z, _, _ = _inputs(B, D)
    sde = sde_lib.subVPSDE(0.1, 20.0, 1000)
    ck = _Checks(f"{policy} B={B} D={D} {prec}")

    def step(m, label, drop, events=None):
        fg = torch.full((m._num_flat,), float("nan"), device=DEV)
        loss = float(fused_dsm_grad(m, sde, _dev(x), flat_grad=fg, t=_dev(t), z=_dev(z), seed=m._rng_seed, step=STEP_DROP if drop else STEP_NODROP,
                                    bucket_events=events))
        guards.check()
        l64, _ = _dsm_ref(B, D, drop, m._rng_seed, torch.float64)
        ck.bound(f"{label}/loss", abs(loss - l64) / l64, 5e-5)
        _check_param_grads(ck, label, m, fg, B, D, drop, prec)

    _, m0, _ = make_model(WEIGHT_SEED, D=D, precision=prec, dropout=0.0)
    m0.train()
    _assert_plan(m0, policy, B, prec)
    step(m0, "nodrop", False)
    _, m, _ = make_model(WEIGHT_SEED, D=D, precision=prec, dropout=DROP_P)
    m.train()
    _assert_plan(m, policy, B, prec)
    step(m, "drop", True)
    if policy != "default":
        SP.force(tuning_env, policy, DPOSER_WGRAD_BATCHED="0")              # split-K weight gradients instead of the one lane launch (bf16x3)
        _assert_plan(m, policy, B, prec, batched=False)
        step(m, "drop_splitk", True)
    if policy == "MID":
        SP.force(tuning_env, policy, DPOSER_SILU_SPLIT_MAX="0")
        _assert_plan(m, policy, B, prec)
        step(m, "drop_silu0", True)
    SP.force(tuning_env, policy)
    _assert_plan(m, policy, B, prec, events=True)                            # the data-parallel form: a HIP event per gradient bucket
    step(m, "drop_bucketed", True, events=m._engine().bucket_events())
    ck.done()


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("policy,B,D", CASES)
def test_sampler_steps_and_prior_loss_vs_float64_oracle(policy, B, D, prec, tuning_env, guards):
    from dposer_amd.algorithms.advanced import sampling, sde_lib
    from dposer_amd.prior import prior_loss
    SP.force(tuning_env, policy)
    cfg, m, p = make_model(WEIGHT_SEED, D=D, precision=prec, dropout=DROP_P)
    _assert_plan(m, policy, B, prec)
    x, _, z, _, _ = _inputs(B, D)
    ck = _Checks(f"{policy} B={B} D={D} {prec}")
    cfg.sampling.corrector = "none"
    fn = sampling.get_sampling_fn(cfg, sde_lib.subVPSDE(0.1, 20.0, 3), (B, D), lambda v: v, 1e-3, device=DEV)
    ref_x = _sampler_ref(B, D)
    for stride in (0, 1):                                                     # both step paths
        _, xs = fn(m, z=_dev(z), seed=SAMPLER_SEED, traj_stride=stride)
        guards.check()
        ck.bound(f"sampler/stride{stride}", rel_err(t2n(xs), ref_x.numpy()), 1e-4)
    sde1k = sde_lib.subVPSDE(0.1, 20.0, 1000)
    for tt, weighted in ((0.31, True), (0.77, False)):
        x0 = _dev(x).requires_grad_(True)
        lp = prior_loss(m, sde1k, x0, tt, weighted=weighted, z=_dev(z))
        lp.backward()
        guards.check()
        ref_l, ref_g = _prior_ref(B, D, tt, weighted)
        ck.bound(f"prior/loss/t{tt}", abs(float(lp.detach()) - ref_l) / abs(ref_l), 2e-4)
        ck.bound(f"prior/grad/t{tt}", rel_err(t2n(x0.grad), ref_g.numpy()), 2e-4)
    ck.done()


@pytest.mark.parametrize("prec", ["fp32", "bf16", "bf16x3"])
@pytest.mark.parametrize("B,D", [(65, 63), (200, 63), (513, 63), (200, 126)])
def test_eval_forward_bits_do_not_depend_on_the_tiling(B, D, prec, tuning_env, guards):
    """Every tiling gives a wave 32 x 32 sub-tiles of the output and walks K in the same order, so the eval forward is bit-identical
    across the 128x32, 128x128 and 256x256 tilings (csrc/scorefc.hip, DPOSER_SMALL_TILE_MAX) in all three precisions."""
    cfg, m, p = make_model(WEIGHT_SEED, D=D, precision=prec, dropout=DROP_P)
    x, _, _, _, labels = _inputs(B, D)
    outs = {}
    for policy in ("default", "MID", "BIG"):
        if policy == "BIG" and SP.model_plan(m, B).padded % 256 != 0:
            continue                                                          # (128 padded samples cannot hold a 256-row tile: the MID case)
        SP.force(tuning_env, policy)
        pl = SP.model_plan(m, B)
        assert (pl.gn, pl.time, pl.final) == _expected_tiles(policy)[0:1] + _expected_tiles(policy)[2:4], (policy, pl)
        with torch.no_grad():
            outs[policy] = m(_dev(x), _dev(labels)).clone()
        guards.check()
    assert torch.isfinite(outs["default"]).all() and float(outs["default"].abs().max()) > 0
    for policy, out in outs.items():
        assert torch.equal(out, outs["default"]), (policy, float((out - outs["default"]).abs().max()))
