"""The training optimizer's kernels (k_sqnorm, k_adam_ema, k_adam_pack: csrc/elementwise.hip) behind the five optimizer entries of the C
ABI, called directly on torch tensors as FusedAdam.fused_step / fused_step_sharded call them, against the float64 oracle of
tests/adam_ref.py: case by case and quantity by quantity (both moments, the parameter step p_new - p_old, the shadow step s_new - s_old,
the squared norm in scratch[0]).  tests/adam_cases.py holds the cases and the band; tests/test_adam_ref_cpu.py pins that oracle to
torch.optim.Adam, measures the band (D32: float32 oracle vs float64 oracle, per case and quantity) and shows that sixteen planted
faults leave it.  Tolerance: 8 x D32, the factor and the reasoning of tests/smplify_cases.py.  What must not change is compared bit
for bit: state inside no-gradient ranges, a guard of 64 floats behind every buffer, everything in a dropped step, and the re-pack
kernel against the two-kernel path.

Measured on an MI355X, the worst distance / D32 per test (the tolerance is 8) stands in the docstring of each test; over the whole file it
is 1.20 (two_trips, the squared norm).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import adam_cases as AC
from dposer_amd import _C
from gpu_common import DEV
from helpers import _log_measured

pytestmark = pytest.mark.gpu

GUARD = 64                  # floats behind every buffer that no call may touch
COUNTER0 = 5.0              # the dropped-step counter scratch[1] before a call
KEYS = ("p", "g", "m", "v", "s")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


class State:
    """p, g, m, v, s of one optimizer call on the device, each followed by its guard, and the scratch block of the call."""

    def __init__(self, x):
        self.n = x["p"].size
        self.guard = np.arange(GUARD, dtype=np.float32) - 7.25
        self.buf = {k: torch.tensor(np.concatenate([x[k], self.guard]), device=DEV) for k in KEYS if x[k] is not None}
        self.scratch = torch.zeros(16384, dtype=torch.float32, device=DEV)
        self.scratch[1] = COUNTER0

    def t(self, k, lo=0, hi=None):
        return None if k not in self.buf else self.buf[k][lo:self.n if hi is None else hi]

    def host(self):
        torch.cuda.synchronize()
        out = {k: (self.buf[k][:self.n].cpu().numpy() if k in self.buf else None) for k in KEYS}
        sc = self.scratch[:2].cpu().numpy()
        out.update(sq=sc[0], counter=float(sc[1]))
        return out

    def guards_intact(self):
        return all(_same_bits(b[self.n:].cpu().numpy(), self.guard) for b in self.buf.values())


def _i64x2(a):
    return (C.c_int64 * 2)(*(list(a) + [0, 0])[:2])


def _hyper_args(h, weight_decay=True):
    return [h["lr"], h["beta1"], h["beta2"], h["eps"]] + ([h["weight_decay"]] if weight_decay else []) + [
        h["grad_clip"], h["grad_scale"], h["step"], h["ema_one_minus_decay"]]


def _step(st, skips, hyper, presummed=0, lo=0, hi=None, entry="dposer_adam_ema_clip_step_wd"):
    """One call on [lo, hi) of the state's buffers (the whole state by default), skips relative to lo."""
    hi = st.n if hi is None else hi
    args = [_C.ptr(st.t(k, lo, hi)) for k in ("p", "g", "m", "v", "s")] + [hi - lo, _i64x2([a for a, _ in skips]), _i64x2([b for _, b in skips]), len(skips)]
    if entry == "dposer_adam_ema_clip_step_wd":
        args += _hyper_args(hyper) + [_C.ptr(st.scratch), presummed, _C.stream_ptr()]
    else:
        assert hyper["weight_decay"] == 0 and presummed == (entry == "dposer_adam_ema_clip_step_presummed")
        args += _hyper_args(hyper, weight_decay=False) + [_C.ptr(st.scratch), _C.stream_ptr()]
    _C.check(getattr(_C.lib(), entry)(*args), entry)


def _sqnorm(st, lo=0, hi=None):
    hi = st.n if hi is None else hi
    _C.check(_C.lib().dposer_grad_sqnorm(_C.ptr(st.t("g", lo, hi)), hi - lo, _C.ptr(st.scratch), _C.stream_ptr()), "dposer_grad_sqnorm")
    return np.float32(st.scratch[0].item())


def _hold_to(got, ref, old, name, what=None):
    """Every quantity of the device's step inside the case's tolerance; -> the worst distance / D32."""
    assert not ref["dropped"]
    dist = AC.distances(got, ref, old)
    ratio, k = AC.worst_ratio(dist, name)
    _log_measured("d32_ratio", ratio)
    print(f"{what or name}: worst {k} = {dist[k]:.2e} = {ratio:.2f} x d32 | " + " ".join(f"{q}={v / AC.D32[name][q]:.2f}" for q, v in dist.items()))
    for q, v in dist.items():
        assert v < AC.TOL[name][q], (what or name, q, v, AC.TOL[name][q])
    return ratio


def _untouched_where_skipped(got, old, skips):
    return all(_same_bits(got[k][lo:hi], old[k][lo:hi]) for lo, hi in skips for k in ("p", "m", "v"))


# ---- a. one step against the float64 oracle ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in AC.CASES if n != "model_d63" and not n.startswith("chain_")])
def test_one_step_matches_the_float64_oracle(name):
    """dposer_adam_ema_clip_step_wd on every case of tests/adam_cases.py: the first step, the clip active / idle / off / tiny (where the
    1e-6 of the coefficient is 2e-4 of the norm), a late step, weight decay under the clip, grad_scale, two no-gradient ranges with ends
    that are no multiples of 4, eps dominating the denominator, no shadow, 2^20 + 7 elements (the second grid-stride trip of both
    kernels and the tail) and n = 1, 3, 4, 5, 255, 256, 257.  scratch[1] stays, the guards and the state inside the no-gradient
    ranges keep their bits.
    Measured, worst distance / d32: two_trips 1.20 (sq), n256 1.10 (m); 1.00 in every other case, set by dp / ds (and m, v where the
    oracle's norm has the kernel's bits), where the kernel's results carry the bits of the float32 oracle; the other quantities at
    0.01 ... 0.95."""
    c, x = AC.CASES[name], AC.inputs(name)
    st = State(x)
    _step(st, c["skips"], c["hyper"])
    got = st.host()
    _hold_to(got, AC.reference(name), x, name)
    assert got["counter"] == COUNTER0 and st.guards_intact() and _same_bits(got["g"], x["g"])
    assert _untouched_where_skipped(got, x, c["skips"])


def test_the_older_entry_is_the_same_step():
    """dposer_adam_ema_clip_step (no weight decay argument) is dposer_adam_ema_clip_step_wd with weight_decay = 0, bit for bit."""
    c, x = AC.CASES["skips"], AC.inputs("skips")
    a, b = State(x), State(x)
    _step(a, c["skips"], c["hyper"])
    _step(b, c["skips"], c["hyper"], entry="dposer_adam_ema_clip_step")
    ga, gb = a.host(), b.host()
    assert all(_same_bits(ga[k], gb[k]) for k in KEYS) and _bits(ga["sq"]) == _bits(gb["sq"]) and gb["counter"] == COUNTER0 and b.guards_intact()


def test_three_chained_steps_match_the_float64_oracle():
    """Steps 1, 2, 3 with the state kept on the device (zero moments first; the clip idle, active, idle): before each step the oracle
    restarts from the device's state, so every step is held to its own band.
    Measured, worst distance / d32: 1.00 in each of the three steps (dp / ds, v in step 2); m 0.16 ... 0.46, sq 0.14 ... 0.51."""
    st = State(AC.inputs("chain_1"))
    for name in ("chain_1", "chain_2", "chain_3"):
        st.buf["g"][:st.n] = torch.tensor(AC.inputs(name)["g"], device=DEV)
        old = st.host()
        _step(st, (), AC.CASES[name]["hyper"])
        got = st.host()
        _hold_to(got, AC.run_oracle(name, state={k: old[k] for k in KEYS}), old, name)
        assert got["counter"] == COUNTER0 and st.guards_intact()


# ---- b. the pre-summed form -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["n1", "n3", "clip_active", "two_trips", "no_clip"])
def test_presummed_norm(name):
    """dposer_grad_sqnorm alone against the float64 sum (n = 1, 3, 1027, 2^20 + 7), then the step with presummed = 1 and that value in
    scratch[0]: inside the band; with the clip off, bit for bit the step that sums the norm itself.
    Measured: dposer_grad_sqnorm at 0.22 (n = 1), 0.10 (3), 0.58 (1027), 1.20 (2^20 + 7), 0.38 (no_clip) x d32; the pre-summed step at 1.00,
    1.00, 1.00, 1.20 (two_trips: sq), 1.00."""
    c, x, ref = AC.CASES[name], AC.inputs(name), AC.reference(name)
    st = State(x)
    sq = _sqnorm(st)
    d = abs(float(sq) - ref["sq"]) / ref["sq"]
    print(f"{name}: dposer_grad_sqnorm {d:.2e} = {d / AC.D32[name]['sq']:.2f} x d32")
    assert d < AC.TOL[name]["sq"] and st.host()["counter"] == COUNTER0
    _step(st, c["skips"], c["hyper"], presummed=1)
    got = st.host()
    assert _bits(got["sq"]) == _bits(sq) and got["counter"] == COUNTER0 and st.guards_intact()
    _hold_to(got, ref, x, name, f"{name} presummed")
    if c["hyper"]["grad_clip"] < 0:
        own = State(x)
        _step(own, c["skips"], c["hyper"])
        want = own.host()
        assert all(_same_bits(got[k], want[k]) for k in KEYS)
    if c["hyper"]["weight_decay"] == 0:          # the entry without the flag
        other = State(x)
        other.scratch[0] = float(sq)
        _step(other, c["skips"], c["hyper"], presummed=1, entry="dposer_adam_ema_clip_step_presummed")
        want = other.host()
        assert all(_same_bits(got[k], want[k]) for k in KEYS)


@pytest.mark.parametrize("clip", [True, False])
def test_three_shards_are_the_unsharded_step(clip):
    """FusedAdam.fused_step_sharded in one process: zero1_bounds(1027, 3), dposer_grad_sqnorm per range summed on the host into
    scratch[0], then one pre-summed call per range on pointers offset into the buffers with the no-gradient ranges of ``skips`` re-based
    as losses.py re-bases them.  Inside the band of the unsharded step's oracle; with the clip off bit for bit the unsharded call.
    Measured, worst distance / d32: 1.00 with and without the clip (ds; v 0.87, m 0.35, the host-summed sq 0.05)."""
    from dposer_amd.distributed import zero1_bounds
    name = "skips"
    c, x = AC.CASES[name], AC.inputs(name)
    hyper = dict(c["hyper"]) if clip else dict(c["hyper"], grad_clip=-1.0)
    bounds = zero1_bounds(AC.N, 3)
    assert bounds == [(0, 344), (344, 688), (688, 1027)]
    st = State(x)
    total = np.float32(0)
    for lo, hi in bounds:
        total = np.float32(total + _sqnorm(st, lo, hi))
    st.scratch[0] = float(total)
    for lo, hi in bounds:
        skips = [(max(a, lo) - lo, min(b, hi) - lo) for a, b in c["skips"] if min(b, hi) > max(a, lo)]
        _step(st, skips, hyper, presummed=1, lo=lo, hi=hi)
    got = st.host()
    assert got["counter"] == COUNTER0 and st.guards_intact() and _untouched_where_skipped(got, x, c["skips"])
    if clip:
        _hold_to(got, AC.reference(name), x, name, "three shards")
    else:
        own = State(x)
        _step(own, c["skips"], hyper)
        want = own.host()
        assert all(_same_bits(got[k], want[k]) for k in KEYS)
        _hold_to(got, AC.run_oracle(name, grad_clip=-1.0), x, name, "three shards, clip off")


# ---- c. dropped steps ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,index,bad", [
    ("clip_active", 0, np.nan), ("clip_active", AC.N - 1, np.nan), ("two_trips", AC.N_TWO_TRIPS - 6, np.nan), ("two_trips", AC.N_TWO_TRIPS - 1, np.nan),
    ("clip_active", 500, np.inf), ("clip_active", 500, 1e20), ("no_clip", 500, -np.inf), ("skips", 1, np.nan)],
    ids=["nan_first", "nan_tail_1027", "nan_second_trip", "nan_tail_two_trips", "inf", "finite_1e20", "minus_inf_no_clip", "nan_skips"])
def test_a_non_finite_gradient_drops_the_step(name, index, bad):
    """A NaN at index 0, in the last element of n = 1027 (the tail path of k_sqnorm), beyond 2^20 (the second trip's float4 and the tail);
    an Inf; a finite entry of 1e20 whose float32 square overflows: every buffer keeps its bits, scratch[1] grows by exactly 1, and the
    next call with the finite gradient is the case's ordinary step and leaves the counter alone."""
    c, x = AC.CASES[name], AC.inputs(name)
    g = np.array(x["g"])
    g[index] = bad
    st = State(dict(x, g=g))
    _step(st, c["skips"], c["hyper"])
    got = st.host()
    assert not np.isfinite(got["sq"])
    assert all(_same_bits(got[k], x[k]) for k in KEYS if k != "g" and x[k] is not None) and _same_bits(got["g"], g), name
    assert got["counter"] == COUNTER0 + 1 and st.guards_intact()
    st.buf["g"][:st.n] = torch.tensor(x["g"], device=DEV)
    _step(st, c["skips"], c["hyper"])
    got = st.host()
    _hold_to(got, AC.reference(name), x, name, f"{name} after a dropped step")
    assert got["counter"] == COUNTER0 + 1 and st.guards_intact()


def test_a_non_finite_presummed_norm_drops_the_step():
    c, x = AC.CASES["clip_active"], AC.inputs("clip_active")
    st = State(x)
    st.scratch[0] = float("inf")
    _step(st, c["skips"], c["hyper"], presummed=1)
    got = st.host()
    assert all(_same_bits(got[k], x[k]) for k in KEYS) and got["counter"] == COUNTER0 + 1 and np.isinf(got["sq"]) and st.guards_intact()


# ---- d. the two-kernel path against the re-pack kernel -----------------------------------------------------------------------------------
CONFIGS = {                                      # the smallest models the library builds: hidden 512, embed 128, one block
    "d63_bf16": (63, _C.EMB_POSITIONAL, _C.PREC_BF16),
    "d65_fp32": (65, _C.EMB_POSITIONAL, _C.PREC_FP32),           # a second, partial K tile in pre_dense and a second row tile in post_dense
    "d63_fourier_bf16": (63, _C.EMB_FOURIER, _C.PREC_BF16),      # two no-gradient ranges
}
# setting -> (magnitudes and hyper-parameters, shadow, pre-summed, dropped)
SETTINGS = {
    "clip_active": (AC.CLIP_ACTIVE, True, False, False), "weight_decay_clip": (AC.WEIGHT_DECAY_CLIP, True, False, False),
    "late_step": (AC.LATE_STEP, True, False, False), "no_ema": (AC.CLIP_ACTIVE, False, False, False),
    "presummed": (AC.CLIP_ACTIVE, True, True, False), "dropped": (AC.CLIP_ACTIVE, True, False, True),
}


@pytest.fixture(scope="module")
def handles():
    lib, out = _C.lib(), {}
    for name, (D, emb, prec) in CONFIGS.items():
        h = C.c_void_p()
        d = _C.ScoreFCDesc(D, AC.MODEL_H, AC.MODEL_E, 1, emb, 1, 1000, prec, 0.1)
        _C.check(lib.dposer_scorefc_create(C.byref(d), C.byref(h)), "dposer_scorefc_create")
        lo, hi = (C.c_int64 * 2)(), (C.c_int64 * 2)()
        k = lib.dposer_scorefc_nograd_ranges(h, lo, hi)
        out[name] = (h, lib.dposer_scorefc_num_params(h), tuple((lo[i], hi[i]) for i in range(k)), lib.dposer_scorefc_packed_bytes(h, 1))
    yield out
    for h, *_ in out.values():
        lib.dposer_scorefc_destroy(h)


def _pack(h, flat, nbytes):
    packed = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    _C.check(_C.lib().dposer_scorefc_pack(h, _C.ptr(flat), _C.ptr(packed), 1, _C.stream_ptr()), "dposer_scorefc_pack")
    return packed


@pytest.mark.parametrize("write_through", [None, "0"], ids=["wt_default", "wt_0"])
@pytest.mark.parametrize("config", list(CONFIGS))
def test_repack_kernel_is_the_two_kernel_path_bit_for_bit(config, write_through, handles, tuning_env):
    """From identical synthetic state over the whole flat buffer (zero gradient inside the no-gradient ranges), path A =
    dposer_adam_ema_clip_step_wd + dposer_scorefc_pack(with_backward = 1) and path B = dposer_scorefc_adam_pack_step end in the same bits:
    parameters, moments, shadow, scratch[0:2] and packed bytes -- with the clip active, weight decay, a late step, no shadow, the
    pre-summed norm, and a dropped step (whose packed bytes are those from before the call); path B with the write-through stores
    (default) and with DPOSER_ADAM_WT=0 (plain stores).  Path A of D = 63 bf16 is the case model_d63 of tests/adam_cases.py and is held
    to the float64 oracle, which carries the oracle over to the re-pack kernel.
    Measured, path A of model_d63, worst distance / d32: 1.00 (ds and dp; v 0.92, m 0.54, sq 0.29)."""
    tuning_env(DPOSER_ADAM_WT=write_through)
    h, n, nograd, nbytes = handles[config]
    assert len(nograd) == (2 if "fourier" in config else 1)
    if config == "d63_bf16":
        assert n == AC.MODEL_N and nograd == (AC.MODEL_COND,)
    lib = _C.lib()
    for setting, (scales, ema, presummed, dropped) in SETTINGS.items():
        c = AC.model_case(n, nograd, scales, ema=ema)
        on_the_case = config == "d63_bf16" and setting == "clip_active"
        x = AC.inputs("model_d63") if on_the_case else AC.draw(c, 7000 + sorted(SETTINGS).index(setting))
        if dropped:
            x = dict(x, g=np.array(x["g"]))
            x["g"][n // 2] = np.nan
        a, b = State(x), State(x)
        if presummed:
            for st in (a, b):
                _sqnorm(st)
        _step(a, nograd, c["hyper"], presummed=int(presummed))
        packed_before = _pack(h, b.t("p"), nbytes)
        packed_b = packed_before.clone()
        _C.check(lib.dposer_scorefc_adam_pack_step(
            h, *[_C.ptr(b.t(k)) for k in KEYS], _C.ptr(packed_b), _i64x2([lo for lo, _ in nograd]), _i64x2([hi for _, hi in nograd]), len(nograd),
            *_hyper_args(c["hyper"]), _C.ptr(b.scratch), int(presummed), _C.stream_ptr()), "dposer_scorefc_adam_pack_step")
        packed_a = _pack(h, a.t("p"), nbytes)
        ga, gb = a.host(), b.host()
        what = f"{config} {setting}"
        for k in KEYS:
            assert (x[k] is None and gb[k] is None) or _same_bits(ga[k], gb[k]), (what, k)
        assert _bits(ga["sq"]) == _bits(gb["sq"]) and ga["counter"] == gb["counter"] == COUNTER0 + (1 if dropped else 0), what
        assert torch.equal(packed_a, packed_b), what
        assert a.guards_intact() and b.guards_intact() and _untouched_where_skipped(gb, x, nograd), what
        if dropped:
            assert torch.equal(packed_b, packed_before) and all(_same_bits(gb[k], x[k]) for k in KEYS), what
        else:
            assert not torch.equal(packed_b, packed_before) and not _same_bits(gb["p"], x["p"]), what
        if on_the_case:
            _hold_to(ga, AC.reference("model_d63"), x, "model_d63")
