"""Float64 reference of the SDE scalars and of the elementwise output stages that consume them, with a first-order fp32 error band
(numpy only).  What tests/test_sde_ref_cpu.py validates on the CPU and tests/test_gpu_sde_sweep.py holds the kernels against.

The scalars (dposer_amd/csrc/sde_dev.h `sde_at`, `make_sde_dev_at`, `used_sigma`; reference sde_lib.py / utils.py / model.py):
    mc, sd       marginal_prob: mean = mc x, std = sd           beta, g   drift -1/2 beta x, diffusion g
    label        what the network is conditioned on             sd_score  the std the score is divided by
for the five kinds  subvp, vp, ve, ve_discrete, vp_discrete.

Exactness.  `t` is an fp32 number and enters exactly.  Every product that decides an INDEX is formed in fp32 as torch forms it on the
CPU -- one rounded multiply (`t * 999`, `t * (N - 1)`), or one rounded subtraction, one rounded multiply and a round-half-even
(`rint((T - t)(N - 1))`) -- so indices are compared exactly, never under a tolerance.  The VP-discrete table is the reference's own
(golden g27), not recomputed.

The band.  Every quantity is a pair (value, bound): the float64 value of the expression and a first-order bound on the error of its fp32
evaluation.  Each fp32 arithmetic operation (and each python-float constant that is rounded to fp32) contributes one unit roundoff
U = 2^-24 relative to its result; each transcendental -- exp, pow, sqrt, and division -- an allowance of TRANS_ULPS = 2 ulp (ulp = 2^-23
relative).  Incoming bounds travel through the float64 derivative of the operation: |d exp(a)| = exp(a) |da|, |d sqrt(a)| = |da| / (2 sqrt a),
|d(a - b)| <= |da| + |db|, so the cancellation of `1 - exp(2 lmc)` at small t amplifies the bound of exp(2 lmc) by exactly 1 / (1 - exp(2 lmc)).
The output stages are written on the same pairs: the scalar bounds reach the outputs through the stage's own derivatives (the analytic
form of a central difference in each scalar) and the stage's own operations add theirs.  A sum of n terms adds k U sum|term| where k is
the longest chain of additions in the kernel; each stage documents how k is counted from the code.

A comparison is per element: |got - value| <= bound  (`ratio` returns |got - value| / bound; a test asserts max ratio <= 1).
"""
import numpy as np

U = 2.0 ** -24          # fp32 unit roundoff
ULP = 2.0 ** -23        # one fp32 ulp, relative
TRANS_ULPS = 2.0        # allowance per expf / powf / sqrtf / division

KINDS = ("subvp", "vp", "ve", "ve_discrete", "vp_discrete")
F32 = np.float32


class E:
    """(value, first-order bound of the fp32 evaluation error), elementwise on float64 arrays."""
    __slots__ = ("v", "e")

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, dtype=np.float64)
        self.e = np.broadcast_to(np.asarray(e, dtype=np.float64), self.v.shape)

    @staticmethod
    def of(x):
        return x if isinstance(x, E) else E(x)

    def _r(self, v, e, trans=False):
        return E(v, e + (TRANS_ULPS * ULP if trans else U) * np.abs(v))

    def __add__(self, o):
        o = E.of(o)
        return self._r(self.v + o.v, self.e + o.e)

    __radd__ = __add__

    def __sub__(self, o):
        o = E.of(o)
        return self._r(self.v - o.v, self.e + o.e)

    def __rsub__(self, o):
        return E.of(o) - self

    def __mul__(self, o):
        o = E.of(o)
        return self._r(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = E.of(o)
        return self._r(self.v / o.v, self.e / np.abs(o.v) + np.abs(self.v) * o.e / (o.v * o.v), trans=True)

    def __rtruediv__(self, o):
        return E.of(o) / self

    def __neg__(self):
        return E(-self.v, self.e)

    def __getitem__(self, i):
        return E(self.v[i], np.broadcast_to(self.e, self.v.shape)[i])


def const(c):
    """A python-float constant that torch / the kernel round to fp32 before use."""
    return E(c, U * abs(c))


def exp(a):
    v = np.exp(a.v)
    return a._r(v, v * a.e, trans=True)


def sqrt(a):
    v = np.sqrt(a.v)
    return a._r(v, a.e / (2.0 * v), trans=True)


def powc(base, t):
    """base ** t, base a constant pair, t exact."""
    v = np.power(base.v, t.v)
    return t._r(v, np.abs(t.v * v / base.v) * base.e + np.abs(v * np.log(base.v)) * t.e, trans=True)


def esum(terms, k, axis=None):
    """Sum of fp32 terms over `axis` along an addition chain of length <= k."""
    e = np.broadcast_to(terms.e, terms.v.shape)
    return E(terms.v.sum(axis=axis), e.sum(axis=axis) + k * U * np.abs(terms.v).sum(axis=axis))


def ratio(got, ref):
    """|got - value| / bound per element (0 / 0 = 0: an exact quantity reproduced exactly)."""
    d = np.abs(np.asarray(got, dtype=np.float64) - ref.v)
    e = np.broadcast_to(ref.e, d.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(d == 0.0, 0.0, d / e)


def ratio_any(got, refs):
    """Per element the smallest ratio over the admissible references (one, or the two sides of an ambiguous index)."""
    refs = refs if isinstance(refs, (list, tuple)) else [refs]
    r = ratio(got, refs[0])
    for ref in refs[1:]:
        r = np.minimum(r, ratio(got, ref))
    return r


def worst(got, refs):
    r = ratio_any(got, refs)
    return float(np.max(r)) if r.size else 0.0


# ---- indices, exactly as torch forms them on the CPU -------------------------------------------------------------------------------
def label_vp(t32, n_minus_1=999):
    """fp32(t * 999) (utils.py:152) / fp32(t * (N - 1)) (utils.py:158): one rounded multiply."""
    return (np.asarray(t32, F32) * F32(n_minus_1)).astype(F32)


def label_ve_discrete(t32, N=1000, T=1.0, half_up=False):
    """torch.round((T - t) * (N - 1)) (utils.py:176-178): a rounded subtraction, a rounded multiply, round-half-even."""
    p = ((F32(T) - np.asarray(t32, F32)).astype(F32) * F32(N - 1)).astype(F32)
    return (np.floor(p.astype(np.float64) + 0.5) if half_up else np.rint(p)).astype(F32)


def sigma_index(label32, num_scales):
    """model.py:159 `t.long()` truncates; the kernels clamp (the reference would raise past the table)."""
    return np.clip(np.trunc(np.asarray(label32, np.float64)).astype(np.int64), 0, num_scales - 1)


# ---- the scalars -------------------------------------------------------------------------------------------------------------------
def scalars(kind, t32, N=1000, T=1.0, beta_0=0.1, beta_1=20.0, sigma_min=0.01, sigma_max=50.0, table=None, label_shift=0,
            half_up=False, sd_score_is_sd=False):
    """dict(mc, sd, beta, g, sd_score: E; label: fp32 array, exact -- under `ve` the pair sigma(t)).  `table`: the VP-discrete
    sqrt_1m_alphas_cumprod (golden g27).  label_shift / half_up / sd_score_is_sd seed the faults of the mutation check."""
    assert kind in KINDS
    t32 = np.asarray(t32, F32)
    t = E(t32)
    if kind in ("ve", "ve_discrete"):
        sig = const(sigma_min) * powc(const(sigma_max / sigma_min), t)                               # sde_lib.py:260,267
        gk = sqrt(const(2.0 * (np.log(sigma_max) - np.log(sigma_min))))
        label = label_ve_discrete(t32, N, T, half_up) + F32(label_shift) if kind == "ve_discrete" else sig
        return dict(mc=E(np.ones_like(t.v)), sd=sig, beta=E(np.zeros_like(t.v)), g=sig * gk, sd_score=sig, label=label)
    b0, db = const(beta_0), E(beta_1 - beta_0, U * (abs(beta_1) + abs(beta_0) + abs(beta_1 - beta_0)))
    lmc = (-0.25 * (t * t)) * db - (0.5 * t) * b0                                                    # sde_lib.py:214
    mc = exp(lmc)
    v = 1.0 - exp(2.0 * lmc)
    sd = v if kind == "subvp" else sqrt(v)                                                           # :216 / :155
    beta = b0 + t * db                                                                               # :207
    if kind == "subvp":
        g = sqrt(beta * (1.0 - exp(const(-2.0 * beta_0) * t - db * (t * t))))                        # :209-210
    else:
        g = sqrt(beta)                                                                               # :149
    out = dict(mc=mc, sd=sd, beta=beta, g=g, sd_score=sd, label=label_vp(t32, 999) + F32(label_shift))
    if kind == "vp_discrete":
        out["label"] = label_vp(t32, N - 1) + F32(label_shift)                                       # utils.py:158
        if not sd_score_is_sd:
            tab = np.asarray(table, np.float64)
            entry = tab[np.clip(np.trunc(out["label"].astype(np.float64)).astype(np.int64), 0, N - 1)]
            out["sd_score"] = E(entry, TRANS_ULPS * ULP * np.abs(entry))                             # :160 (the table's bound: 2 ulp of the fixture)
    return out


def used_sigma(sigmas32, label, fourier, scale_by_sigma=True, side=0):
    """model.py:152 (Fourier: the label itself) / :159 (sigmas[label.long()]); 1 without scale_by_sigma.  `side` = -1 / +1: the index from
    the lower / upper end of the label's band -- the continuous VE kind, whose index trunc(sigma(t)) is decided by a powf, is compared
    against both (`worst` takes a list) where `ambiguous_index` holds; every other label is exact and has one index."""
    lab = label.v + side * label.e if isinstance(label, E) else np.asarray(label, np.float64)
    if not scale_by_sigma:
        return E(np.ones_like(lab))
    if fourier:
        return label if isinstance(label, E) else E(lab)
    return E(np.asarray(sigmas32, np.float64)[sigma_index(lab, len(sigmas32))])


def ambiguous_index(label):
    """Under the continuous VE kind the index is trunc(sigma(t)), decided by a transcendental: True where the band of sigma(t) holds an integer."""
    if not isinstance(label, E):
        return np.zeros(np.shape(label), dtype=bool)
    return np.floor(label.v - label.e) != np.floor(label.v + label.e)


def _col(s, nd=1):
    """Scalars of a per-row t [G] as columns against [G, C] (nd = 1) or [G, B, D] (nd = 2)."""
    ix = (Ellipsis,) + (None,) * nd
    return {k: (v[ix] if isinstance(v, E) and v.v.ndim else v) for k, v in s.items()}


def _sum_axes(x0, per_row):
    """(axis of the sums, B, D): everything of one shared-t call [B, D]; per row of [G, C]; per leading index of [G, B, D]."""
    sh = np.shape(x0)
    if not per_row:
        return None, sh[-2], sh[-1]
    return (-1, 1, sh[-1]) if len(sh) == 2 else ((-2, -1), sh[-2], sh[-1])


def _score(kind, model, sd_score):
    return model if kind in ("ve", "ve_discrete") else -model / sd_score                             # utils.py:162 / :180


def chain_blocked(n_terms, per_thread=1, cap=1024):
    """Longest addition chain of a blocked loss: serial terms per thread in the grid-stride loop (grid = min(cap, ceil(n / 256)) blocks of
    256) + 6 shuffle levels + 3 cross-wave additions (block_sum_256), then k_sum_partials over <= cap partials: <= ceil(cap / 256)
    serial + 6 + 3."""
    blocks = min(cap, max(1, -(-n_terms // 256)))
    serial = per_thread * -(-n_terms // (256 * blocks))
    return serial + 9 + -(-blocks // 256) + 9


# ---- output stages -----------------------------------------------------------------------------------------------------------------
def out_model(c, usig):
    """k_out_model (model.py:192-194): res / used_sigma per sample (usig as a column against [B, D])."""
    return E(c) / usig


def denoise(kind, s, usig, x0, z, c, weighted, inv_n, ignore_weighted=False, per_row=False):
    """k_perturb_shared + k_denoise at one shared t (completion.py:105-110,131-149): x_t, x0_hat, grad, loss.
    Loss chain: chain_blocked(B D) -- one term per loop pass.  per_row (here and below): every row is a problem of its own with its own
    t (scalars as columns, `_col`), the sums run over the row."""
    xt = s["mc"] * E(x0) + s["sd"] * E(z)
    score = _score(kind, E(c) / usig, s["sd_score"])
    sigma2 = s["sd"] * s["sd"]
    x0h = (xt + sigma2 * score) / s["mc"]
    w = 0.5 * sqrt(1.0 + s["mc"] / sqrt(sigma2)) if (weighted or ignore_weighted) else E(0.5)
    diff = E(x0) - x0h
    axis, B, D = _sum_axes(x0, per_row)
    loss = esum(w * (diff * diff), chain_blocked(B * D), axis=axis) * const(inv_n)
    return dict(x_t=xt, x0_hat=x0h, grad=((2.0 * w) * diff) * const(inv_n), loss=loss)


def ddim(kind, ss, usigs, x0, z, c, weighted, inv_n, weight_at_last=False, per_row=False):
    """k_perturb_shared + n x k_ddim_step (completion.py:112-149): ss / usigs are the scalars / used sigmas at time_traj[0..n]; the weight
    comes from time_traj[0].  Loss chain: chain_blocked(Bpad Dpad / 4, 4 terms per loop pass)."""
    x = ss[0]["mc"] * E(x0) + ss[0]["sd"] * E(z)
    for i in range(len(ss) - 1):
        a, b = ss[i], ss[i + 1]
        score = _score(kind, E(c) / usigs[i], a["sd_score"])
        noise = -score * a["sd"]
        x = (b["mc"] / a["mc"]) * (x - a["sd"] * noise) + b["sd"] * noise
    s0 = ss[-2] if weight_at_last else ss[0]
    w = 0.5 * sqrt(1.0 + s0["mc"] / s0["sd"]) if weighted else E(0.5)
    diff = E(x0) - x
    axis, B, D = _sum_axes(x0, per_row)
    loss = esum(w * (diff * diff), chain_blocked(B * ((D + 3) // 4), per_thread=4), axis=axis) * const(inv_n)
    return dict(x0_hat=x, grad=((2.0 * w) * diff) * const(inv_n), loss=loss)


def red_diff(kind, s, usig, x0, z, c, per_row=False, inv_batch=None):
    """k_red_diff (motion_denoising.py:145-154): eps_pred, grad, loss.  Loss chain: chain_blocked(B ceil(D / 4), 4 terms per pass)."""
    axis, B, D = _sum_axes(x0, per_row)
    score = _score(kind, E(c) / usig, s["sd_score"])
    eps = -score * s["sd"]
    dz = eps - E(z)
    weight = sqrt(s["sd"] * s["sd"]) / s["mc"]
    inv_b = const(1.0 / B if inv_batch is None else inv_batch)
    tot = esum(dz * E(x0), chain_blocked(B * ((D + 3) // 4), per_thread=4), axis=axis)
    wrow = E(weight.v.reshape(tot.v.shape), weight.e.reshape(tot.v.shape)) if per_row else weight
    loss = (wrow * tot) * inv_b
    return dict(eps_pred=eps, grad=(weight * dz) * inv_b, loss=loss)


def em_update(kind, s, s_next, usig, x, c, z, N=1000, pf=False, obs=None, mask=None, z_imp_b=None, z_imp_a=None, pf_factor=0.5):
    """k_em_update (sampling.py:186-187, sde_lib.py:98-104, imputation sampling.py:416-420): x_mean and the new x; with an observation the
    imputation at t after the step and -- s_next given -- the one at t_next ahead of the next predictor call."""
    x = E.of(x)
    score = _score(kind, E(c) / usig, s["sd_score"])
    drift = (-0.5 * s["beta"]) * x
    drift = drift - ((s["g"] * s["g"]) * score) * (pf_factor if pf else 1.0)
    x_mean = x + drift * const(-1.0 / N)
    xn = x_mean if pf else x_mean + (s["g"] * const(np.sqrt(1.0 / N))) * E.of(z)
    if obs is not None:
        m = E(mask)
        xn = xn * (1.0 - m) + (s["mc"] * E(obs) + E(z_imp_b) * s["sd"]) * m
        if s_next is not None:
            xn = xn * (1.0 - m) + (s_next["mc"] * E(obs) + E(z_imp_a) * s_next["sd"]) * m
    return dict(x_mean=x_mean, x=xn)


def langevin(kind, s, usig, x, c, noise, snr, alpha):
    """k_langevin_norms + k_sum_partials2 + k_langevin_update (sampling.py:282-302) on [..., B, D] (c given per row): the two norm sums,
    x_mean and x.  Chains: ||.||^2 of a row is one thread's serial sum, D terms; the batch sum is one sample per thread (B <= 256 x 1024)
    (1 addition) + 6 shuffle levels + 3 cross-wave additions, then k_sum_partials2: <= 4 serial + 6 + 3: 1 + 6 + 3 + 4 + 6 + 3 = 23.
    x_mean = x + step * g and x = x_mean + nscale * n end in one addition whose addend is small against x: the kernel's own half-ulp
    rounding of that addition is up to U |x|, which is also nearly the whole band there -- measured ratios up to 0.999 are that
    rounding, attained, not a fault that is nearly seen (the same holds for the x_mean of em_update)."""
    B, D = np.shape(x)[-2:]
    g = _score(kind, E(c) / usig, s["sd_score"])
    n = E(noise)
    gsum = esum(sqrt(esum(g * g, D, axis=-1)), 23, axis=-1)
    nsum = esum(sqrt(esum(n * n, D, axis=-1)), 23, axis=-1)
    inv_b = const(1.0 / B)
    r0 = (const(snr) * (nsum * inv_b)) / (gsum * inv_b)
    step = ((r0 * r0) * 2.0) * const(alpha)
    nscale = sqrt(step * 2.0)
    x_mean = E(x) + step[..., None, None] * g
    return dict(gsum=gsum, nsum=nsum, x_mean=x_mean, x=x_mean + nscale[..., None, None] * n)


def completion_update(kind, s, usig, x, z, c, obs, mask, m0, v0, weighted, w_prior, w_data, lr, beta1, beta2, eps, k=1):
    """k_perturb_shared + k_completion_update: Adam step number k of DPoserComp.optimize (completion.py:131-149, 195-201; torch.optim.Adam)
    from the moments m0, v0 -- the new x, m and v.  No sums."""
    B, D = np.shape(x)[-2:]
    x, mk = E(x), E(mask)
    xt = s["mc"] * x + s["sd"] * E(z)
    score = _score(kind, E(c) / usig, s["sd_score"])
    sigma2 = s["sd"] * s["sd"]
    x0h = (xt + sigma2 * score) / s["mc"]
    w = 0.5 * sqrt(1.0 + s["mc"] / sqrt(sigma2)) if weighted else E(0.5)
    inv_n = const(1.0 / (B * D))
    g = (((2.0 * w) * (x - x0h)) * inv_n) * const(w_prior) + (((2.0 * (x * mk - E(obs) * mk)) * inv_n) * const(w_data)) * mk
    m = E(m0) + (g - E(m0)) * const(1.0 - beta1)
    v = E(v0) * const(beta2) + const(1.0 - beta2) * (g * g)
    denom = sqrt(v) / const(np.sqrt(1.0 - beta2 ** k)) + const(eps)
    return dict(x=x - const(lr / (1.0 - beta1 ** k)) * (m / denom), m=m, v=v)


def dsm_chains(B, D):
    """(loss chain, column-sum chain) of k_dsm and the two reductions behind it, counted from the code.  A thread keeps one channel
    quad for its samples: lanes = 256 / (Cp / 4) sample lanes per block, g = min(1024, ceil(Bpad / lanes)) blocks, so a thread walks
    S = ceil(Bpad / (g lanes)) samples (Bpad <= B + 512 taken for the bound).
    Loss: 4 S serial terms (`acc += e * e`, four channels per sample) + 6 shuffle levels + 3 cross-wave additions (block_sum_256), then
    the g partials in k_sum_partials' order: ceil(g / 256) serial + 6 + 3.
    Column sums of dres: S serial (`csum += `) + `lanes` additions (the block's sample lanes in turn) + reduce_job_body over the g
    partial rows: g <= 64 rows serially, else ceil(g / 64) per accumulator + 3 pair levels + 8 slices (+ 1: the first addition to 0)."""
    cp = -(-D // 64) * 64
    lanes = 256 // (cp // 4)
    bpad = B + 512
    g = min(1024, -(-bpad // lanes))
    S = -(-bpad // (g * lanes))
    return 4 * S + 9 + -(-g // 256) + 9, S + lanes + (g if g <= 64 else -(-g // 64) + 12)


def dsm(kind, s, usig, c, z, chains=None):
    """k_dsm behind a network whose output is c (losses.py:121-131, utils.py:162 / :180), rows with a t of their own (scalars as columns):
    e = score std + z, loss = mean(e^2), dres = d loss / d res per element, and its column sums -- the gradient of post_dense.bias.
    The perturbation of k_prep_train (x_t = mc x0 + std z) only feeds the network, so behind a constant network it is not observable."""
    z = E.of(z)
    B, D = z.v.shape[-2:]
    k_loss, k_cs = chains or dsm_chains(B, D)
    sd = s["sd"]
    e = _score(kind, E(c) / usig, sd) * sd + z
    gs = const(1.0 / (B * D))
    loss = esum(e * e, k_loss) * gs
    dres = (((2.0 * e) * sd) * gs) / usig if kind == "ve" else ((-2.0 * e) * gs) / usig
    return dict(loss=loss, dres=dres, bias_grad=esum(dres, k_cs, axis=-2))


def pf_rhs(kind, s, x, out, noise=None, dx=None):
    """k_pf_rhs_begin / _end (likelihood.py:60-65, 86-95): dout, drift and the Hutchinson term per row.  Row chain: ceil(D / 64) serial
    terms per lane + 6 shuffle levels."""
    ve = kind == "ve"
    g2 = s["g"] * s["g"]
    a = E(np.zeros(())) if ve else -0.5 * s["beta"]
    score = E(out) if ve else (-E(out)) / s["sd"]
    res = dict(drift=a * E(x) - (g2 * score) * 0.5)
    if noise is not None:
        gscore = ((-E(noise)) * 0.5) * g2
        res["dout"] = gscore if ve else -(gscore / s["sd"])
        if dx is not None:
            vjp = E(dx) + E(noise) * a
            res["hutch"] = esum(vjp * E(noise), -(-np.shape(x)[-1] // 64) + 6, axis=-1)
    return res


# ---- the time values of the sweeps --------------------------------------------------------------------------------------------------
def boundary_times(mult, ks=(0, 1, 2, 4, 5, 499, 500, 998, 999), T=1.0, eps=1e-5):
    """For every k the two adjacent fp32 t with fp32(t * mult) < k <= fp32(t * mult), kept inside [eps, T]: k = 0 has no lower side
    at t > 0, and past T only the clamp would answer."""
    out = []
    for k in ks:
        t = F32(k / float(mult))
        while (t * F32(mult)).astype(F32) >= k and t > 0:
            t = np.nextafter(t, F32(-1))
        while (t * F32(mult)).astype(F32) < k:
            t = np.nextafter(t, F32(2))
        out += [np.nextafter(t, F32(-1)), t]                 # product just below k, product k or just above
    out = np.asarray(out, F32)
    return np.unique(out[(out >= F32(eps)) & (out <= F32(T))])


def half_times(N=1000, T=1.0, want=4):
    """fp32 t with fp32(fp32(T - t) * (N - 1)) = k + 0.5 EXACTLY, `want` of them for even and `want` for odd k: where round-half-even and
    round-half-up part (VE-discrete label)."""
    found = {0: [], 1: []}
    for k in range(1, N - 1):
        if len(found[k % 2]) >= want:
            continue
        t = F32(T - (k + 0.5) / (N - 1))
        for c in [t] + [np.nextafter(t, F32(s)) for s in (-1, 2)]:
            if ((F32(T) - c).astype(F32) * F32(N - 1)).astype(F32) == F32(k + 0.5):
                found[k % 2].append(c)
                break
    return np.asarray(found[0] + found[1], F32)
