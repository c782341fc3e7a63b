"""The cases, the distances and the comparison band of the fused Adam / clip / EMA optimizer step (k_sqnorm, k_adam_ema, k_adam_pack:
csrc/elementwise.hip) -- shared by tests/test_adam_ref_cpu.py (which pins the oracle tests/adam_ref.py to torch, measures the band and
shows that every planted fault leaves it) and tests/test_gpu_optimizer.py (which holds the kernels to it).  Test infrastructure; numpy
only, no GPU.

Every case is ONE optimizer step from a synthetic state.  Magnitudes are drawn as sign x U(0.5, 1.5) x scale: no entry is near zero,
so every float32 quantity stays in the normal range (denormal second moments are not what these tests pin) and Adam's sign-like
update has no coin-flip coordinates.  The last three gradient entries are 20 x the others: the n % 4 tail of k_sqnorm carries about
half of the squared norm.
"""
import functools

import numpy as np

import adam_ref as AR

N = 1027                            # not a multiple of 4, more than four blocks of 256
N_TWO_TRIPS = AR.TRIP + 7           # the smallest size at which k_sqnorm and k_adam_ema run a second grid-stride trip and the tail
SMALL_N = (1, 3, 4, 5, 255, 256, 257)       # the n < 4 launch and the vector / tail boundary
# the smallest score network the library builds (hidden 512, embed 128, one block, D = 63, positional): its flat parameter count and
# its no-gradient range (pre_dense_cond), csrc/scorefc.hip dposer_scorefc_create; tests/test_gpu_optimizer.py checks both against the handle
MODEL_H, MODEL_E, MODEL_D = 512, 128, 63
_BLOCK = MODEL_H * MODEL_H + MODEL_H + MODEL_H * MODEL_E + MODEL_H + 2 * MODEL_H
MODEL_COND = (MODEL_H * MODEL_D + MODEL_H + MODEL_H * MODEL_E + MODEL_H, MODEL_H * MODEL_D + MODEL_H + MODEL_H * MODEL_E + MODEL_H + MODEL_H * MODEL_H + MODEL_H)
MODEL_N = (MODEL_COND[1] + 2 * MODEL_H + MODEL_E * MODEL_E + MODEL_E + 2 * _BLOCK + MODEL_D * MODEL_H + MODEL_D)

HYPER = dict(lr=2e-4, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, grad_clip=1.0, grad_scale=1.0, step=3, ema_one_minus_decay=0.1)


def _case(n=N, p=3e-2, g=1e-2, m=None, v=None, s_off=0.0, ema=True, skips=(), tail=20.0, after=None, **hyper):
    """p, g: magnitude scales; m / v: scales of the moments (None: zero moments); s_off: scale of s - p (0: s == p); after: the case
    whose float32 oracle result is this case's p, m, v, s (a chain of steps)."""
    assert set(hyper) <= set(HYPER), hyper
    return dict(n=n, p=p, g=g, m=m, v=v, s_off=s_off, ema=ema, skips=tuple(skips), tail=tail, after=after, hyper=dict(HYPER, **hyper))


# the settings several cases (and the model-sized runs of the GPU test) share
CLIP_ACTIVE = dict(g=0.45, m=2e-2, v=4e-4, s_off=1e-3)                                   # norm about 20 x the clip
WEIGHT_DECAY_CLIP = dict(p=1.0, g=0.45, m=5e-2, v=2.5e-3, s_off=1e-2, weight_decay=0.05, lr=0.03)
LATE_STEP = dict(g=1e-2, m=1e-2, v=1e-4, s_off=1e-2, step=200000, ema_one_minus_decay=1e-4)

CASES = {
    "first_step": _case(step=1, ema_one_minus_decay=9.0 / 11.0),                          # zero moments, s == p, norm 0.48 < clip
    "clip_active": _case(**CLIP_ACTIVE),
    "tiny_clip": _case(p=2e-4, g=1e-4, m=2e-5, v=4e-10, s_off=1e-5, grad_clip=1e-3, step=2),      # norm 4.8e-3: the 1e-6 is 2e-4 of it
    "no_clip": _case(g=5.0, m=5.0, v=25.0, s_off=1e-3, grad_clip=-1.0),
    "late_step": _case(**LATE_STEP),
    "weight_decay_clip": _case(**WEIGHT_DECAY_CLIP),
    "grad_scale": _case(g=8 * 0.45, m=2e-2, v=4e-4, s_off=1e-3, grad_scale=0.125),
    "skips": _case(g=1e-2, m=1e-2, v=1e-4, s_off=1e-2, skips=((5, 130), (N - 301, N - 2)), ema_one_minus_decay=0.5),
    "eps_dominates": _case(p=1e-4, g=1e-9, m=1e-9, v=1e-18, s_off=1e-5, grad_clip=-1.0, step=2),
    "no_ema": _case(ema=False, **CLIP_ACTIVE),
    # 2^20 entries of 0.02 (squared norm about 450) and seven of 3 from 2^20 on (63: an eighth of the total), four of them in the
    # second trip's only float4 and three in the tail
    "two_trips": _case(n=N_TWO_TRIPS, g=2e-2, m=1e-3, v=1e-6, s_off=1e-3, tail=1.0),
    # three chained steps from zero moments: the clip idle, active, idle
    "chain_1": _case(step=1), "chain_2": _case(g=3e-2, step=2, after="chain_1"), "chain_3": _case(g=3e-3, step=3, after="chain_2"),
}


def model_case(n, skips, settings, ema=True):
    """One of the shared settings over a whole flat parameter buffer of about 1 M entries: gradient entries of 0.02 (norm about 20 x the
    clip), 9 in the last three."""
    return _case(n=n, skips=skips, ema=ema, **dict(settings, g=2e-2, tail=450.0))


CASES["model_d63"] = model_case(MODEL_N, (MODEL_COND,), CLIP_ACTIVE)
for _n in SMALL_N:
    CASES[f"n{_n}"] = _case(n=_n, **CLIP_ACTIVE)
QUANTITIES = ("m", "v", "dp", "ds", "sq")


def draw(c, seed, two_trips=False):
    """dict of float32 numpy arrays p, g, m, v, s (None without a shadow) of the case description ``c``."""
    n = c["n"]
    rs = np.random.RandomState(seed)
    f32 = lambda a: np.asarray(a, dtype=np.float32)
    mag = lambda scale: rs.choice([-1.0, 1.0], n) * rs.uniform(0.5, 1.5, n) * scale
    p, g = f32(mag(c["p"])), mag(c["g"])
    g[-3:] *= c["tail"]
    if two_trips:
        g[AR.TRIP:] = np.sign(g[AR.TRIP:]) * rs.uniform(2.5, 3.5, n - AR.TRIP)
    m = f32(np.zeros(n) if c["m"] is None else mag(c["m"]))
    v = f32(np.zeros(n) if c["v"] is None else np.abs(mag(c["v"])))
    s = f32(p + mag(c["s_off"])) if c["ema"] else None
    for lo, hi in c["skips"]:
        g[lo:hi] = 0.0                                   # as the callers guarantee
    return dict(p=p, g=f32(g), m=m, v=v, s=s)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """The case's state, read-only: drawn from a seed of its own, or (``after``) the float32 oracle's result of the case before it
    with a gradient of its own."""
    c = CASES[name]
    out = draw(c, 4100 + sorted(CASES).index(name), two_trips=name == "two_trips")
    if c["after"]:
        prev = run_oracle(c["after"], np.float32)
        out.update({k: prev[k] for k in ("p", "m", "v", "s")})
    for a in out.values():
        if a is not None:
            a.setflags(write=False)
    return out


def run_oracle(name, dtype=np.float64, mutation=None, state=None, sq=None, **hyper):
    """The oracle's step of a case (``state``: other p, g, m, v, s than the case's own; ``hyper``: overrides)."""
    c, x = CASES[name], dict(inputs(name), **(state or {}))
    return AR.adam_step(x["p"], x["g"], x["m"], x["v"], x["s"], c["skips"], dtype=dtype, mutation=mutation, sq=sq, **dict(c["hyper"], **hyper))


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 oracle of a case: computed once per process, shared, never written to."""
    out = run_oracle(name)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def _rel_max(a, b):
    """Largest |a - b| over largest |b|; anything non-finite is infinitely far."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    if not np.isfinite(a).all():
        return float("inf")
    return float(np.abs(a - b).max() / np.abs(b).max())


def distances(got, ref, old):
    """The compared quantities of one step against a reference step from the same state ``old`` (float32 p and s): m, v: largest
    difference over the largest reference entry; dp = p_new - p_old, ds = s_new - s_old: the same measure on the differences, taken in
    float64 (what makes the update and the EMA step visible at all next to the values they move); sq: relative."""
    d64 = lambda a: np.asarray(a, dtype=np.float64)
    out = {"m": _rel_max(got["m"], ref["m"]), "v": _rel_max(got["v"], ref["v"]),
           "dp": _rel_max(d64(got["p"]) - d64(old["p"]), d64(ref["p"]) - d64(old["p"])),
           "sq": _rel_max(np.float64(got["sq"]).reshape(1), np.float64(ref["sq"]).reshape(1))}
    if ref["s"] is not None:
        out["ds"] = _rel_max(d64(got["s"]) - d64(old["s"]), d64(ref["s"]) - d64(old["s"]))
    return out


# ---- the band.  D32[case][quantity]: the distance of the float32 oracle from the float64 oracle, MEASURED by
# tests/test_adam_ref_cpu.py::test_float32_oracle_stays_inside_the_band (which prints the table and asserts that a fresh measurement stays
# within 2 x of these constants): D32_MEASURED holds the values as measured, D32 gives each a floor of 2^-23 (one float32 ulp of the largest entry: a one-ulp
# device function must not fail a quantity the float32 oracle happened to hit exactly).  TOL = 8 x D32, the factor and the reasoning of
# tests/smplify_cases.py: one float32 run is one sample of rounding noise; the kernels differ from it by the summation order of the norm
# and by 1-2 ulp device functions.  The band is per case: ds where s == p or 1 - decay = 1e-4 is legitimately resolved far more coarsely
# than elsewhere (s moves by a few ulp of itself), and a maximum over the cases would blind every other case.
FLOOR = 2.0 ** -23
D32_MEASURED = {
    "first_step": dict(m=1.41e-08, v=3.47e-08, dp=9.05e-06, ds=6.79e-06, sq=5.18e-08),
    "clip_active": dict(m=6.72e-08, v=8.71e-08, dp=2.42e-05, ds=1.30e-05, sq=6.93e-08),
    "tiny_clip": dict(m=1.88e-07, v=2.24e-07, dp=2.81e-07, ds=1.55e-06, sq=1.13e-07),
    "no_clip": dict(m=4.03e-08, v=8.97e-08, dp=1.81e-05, ds=1.33e-05, sq=3.76e-08),
    "late_step": dict(m=2.08e-08, v=9.69e-08, dp=3.54e-06, ds=1.22e-03, sq=5.34e-08),
    "weight_decay_clip": dict(m=3.94e-08, v=6.97e-08, dp=4.92e-06, ds=2.60e-05, sq=2.15e-08),
    "grad_scale": dict(m=8.09e-08, v=7.95e-08, dp=1.97e-05, ds=1.32e-05, sq=1.32e-08),
    "skips": dict(m=4.22e-08, v=1.03e-07, dp=2.31e-05, ds=3.71e-07, sq=6.72e-08),
    "eps_dominates": dict(m=4.75e-08, v=7.54e-08, dp=2.15e-07, ds=9.67e-07, sq=1.94e-08),
    "no_ema": dict(m=5.38e-08, v=7.57e-08, dp=1.79e-05, sq=6.42e-08),
    "two_trips": dict(m=8.09e-08, v=1.78e-07, dp=1.37e-05, ds=1.30e-05, sq=2.64e-08),
    "chain_1": dict(m=3.97e-08, v=3.18e-08, dp=4.22e-06, ds=5.62e-05, sq=1.71e-08),
    "chain_2": dict(m=5.49e-08, v=1.38e-07, dp=9.39e-06, ds=5.36e-05, sq=5.59e-08),
    "chain_3": dict(m=1.86e-08, v=5.57e-08, dp=1.01e-05, ds=3.87e-05, sq=6.05e-08),
    "model_d63": dict(m=6.47e-08, v=1.09e-07, dp=1.69e-05, ds=1.30e-05, sq=3.45e-08),
    "n1": dict(m=4.63e-08, v=2.77e-08, dp=1.25e-05, ds=2.24e-06, sq=2.66e-08),
    "n3": dict(m=1.39e-07, v=1.55e-07, dp=1.20e-05, ds=3.28e-06, sq=1.19e-08),
    "n4": dict(m=3.59e-08, v=5.37e-08, dp=1.54e-05, ds=1.82e-05, sq=2.81e-08),
    "n5": dict(m=8.67e-08, v=5.02e-08, dp=1.52e-05, ds=7.63e-06, sq=4.14e-08),
    "n255": dict(m=2.93e-08, v=9.25e-08, dp=1.35e-05, ds=1.36e-05, sq=2.18e-08),
    "n256": dict(m=8.37e-08, v=1.11e-07, dp=1.52e-05, ds=1.33e-05, sq=2.53e-08),
    "n257": dict(m=9.46e-08, v=1.52e-07, dp=1.64e-05, ds=1.26e-05, sq=8.90e-08),
}
D32 = {name: {q: max(x, FLOOR) for q, x in d.items()} for name, d in D32_MEASURED.items()}
TOL_FACTOR = 8.0
TOL = {name: {q: TOL_FACTOR * x for q, x in d.items()} for name, d in D32.items()}


def worst_ratio(dist, name):
    """(largest distance / D32 over the quantities of the case, its name)."""
    k = max(dist, key=lambda q: dist[q] / D32[name][q])
    return dist[k] / D32[name][k], k
