"""Rounding-faithful float64 oracle of ``ScoreModelFC`` in bf16 mode (test infrastructure; may import ``oracle/``).

The bf16 mode's distance to the plain oracle (4.8e-3 forward) is not noise: it is a fixed set of bf16 stores.  This module restates
the network in float64 and rounds to bf16 exactly where the kernels store bf16, so that what is left between the kernels and this
oracle is the kernels' fp32 arithmetic -- unless one of the roundings falls the other way ("flips"), which then cascades through
the later roundings up to the rounding-noise level.  A batch therefore splits into *clean* rows (no flip anywhere: agreement at fp32
accuracy) and *flipped* rows (agreement at the designed-error level); ``check_rows`` is the rule the GPU tests apply, ``RECORD`` holds
the reference-only numbers (``arith=float32`` against ``arith=float64``) that its bounds are derived from.

Rounding points (read off ``scorefc.hip``, ``epilogues.h``, ``elementwise.hip`` and ``gemm_wgrad_tr.h``; the same table is in
DESIGN.md section 5).  Every store is round-to-nearest-even of an fp32 register (``(__bf16)f`` / ``f32_to_bf16_bits``, common.h), so
the oracle rounds through fp32 as well.  ``skip=<name>`` leaves one of them out, ``rounding="trunc"`` truncates at all of them.

  name    quantity                                   producer                               stored   consumer
  ------  -----------------------------------------  -------------------------------------  -------  ----------------------------------------------
  arg     label * f_k of the sinusoidal embedding    temb_from_freq (k_prep_*, k_time_embed) fp32     sin / cos of both time paths (the one fp32 point:
                                                                                                     the reference forms this product in fp32 too)
  rev     arg * (1 / 2 pi), per-sample-t path only   temb_from_freq<FAST> (k_prep_*)        fp32     v_sin_f32 / v_cos_f32, which take revolutions
  w       every GEMM weight matrix, W and W^T        k_pack (pack_chunk<__bf16>)            bf16     all forward / dgrad GEMMs of the per-sample-t path;
          (shared-t: the x-path matrices only)                                                       shared-t: W_x of the layers and post_dense
  xin     network input x (x_t of the prior loss,    k_prep_infer / k_prep_train /          bf16     layer-0 GEMM; wgrad of pre_dense
          the sampler state)                         k_perturb_shared / k_em_update /
                                                     k_pack_rows (store_quad_ft<__bf16>)
  emb     sinusoidal embedding of the label          k_prep_infer / k_prep_train            bf16     shared_time_embed GEMM; its wgrad
  upre    u = emb W_se^T + b_se (training layout)    EpiBiasSiLU<__bf16, true> (p.pre)      bf16     silu'(u) of the time-branch dgrad
  temb    SiLU(u)                                    EpiBiasSiLU<__bf16>                    bf16     K-concatenated operand of every layer GEMM; wgrad of W_t
  h<l>    output of GroupNorm layer l                EpiGN<__bf16> (TileIO store of o)      bf16     next layer GEMM, residual input of layer l + 2,
          = [h<l-2> +] Drop(SiLU(GN(.)))                                                             post_dense, wgrad operand
  xhat    normalised activation (training layout)    EpiGN<__bf16, true> (p.xhat)           bf16     EpiGNBwd: a = gamma xhat + beta, dgamma, the two means
  dres    d out / used_sigma                         k_dres_from_dout / k_dsm               bf16     dgrad through post_dense, its wgrad, its bias (k_colsum)
  carry   gradient on the residual connection        EpiGNBwd (p.carry_out, even layers)    bf16     EpiGNBwd of layer l - 2 (added to the accumulator)
  dy      gradient w.r.t. the layer's GEMM output    EpiGNBwd (p.dy)                        bf16     dgrad of the layer below, dx, time-branch dgrad, wgrads
  dU      dtemb * silu'(u)                           EpiSiLUBwd / k_silu_bwd_reduce         bf16     wgrad of W_se; bias of shared_time_embed where the
                                                                                                     reduce pass sums the STORED values (``se_bias_stored``)

Kept in fp32 by the kernels and therefore exact here: GEMM accumulators, all biases, GroupNorm statistics, rstd (GnAux), gamma / beta,
the dropout decisions, SiLU and its derivative, the division by ``used_sigmas``, the post_dense output, dx, the parameter-gradient sums
(dgamma / dbeta / layer biases are summed from the fp32 values BEFORE dy is rounded) and, on the shared-t path, the whole time branch
(``build_time_table``: fp32 embedding, fp32 weights, fp32 MFMAs -> an fp32 bias row per layer).
"""
import functools
import math

import numpy as np
import torch

from oracle import score_ref as R

H, E = 1024, 512                     # the shipped widths (hidden 512 / 2048 are out of scope: other epilogues)
BACKWARD_POINTS = ("upre", "xhat", "dres", "carry", "dy", "dU")


def point_names(n_blocks):
    """Every name ``skip=`` accepts for a network of this depth (per-sample-t path)."""
    return ("arg", "rev", "w", "xin", "emb", "temb") + tuple(f"h{l}" for l in range(1 + 2 * n_blocks)) + BACKWARD_POINTS


def round_bf16(v, mode="rne"):
    """fp32 register -> bf16 store -> value, in ``v``'s dtype.  ``rne``: what the kernels do; ``trunc``: the mutation."""
    f = v.to(torch.float32)
    if mode == "rne":
        q = f.to(torch.bfloat16).to(torch.float32)
    elif mode == "trunc":
        q = (f.contiguous().view(torch.int32) & -65536).view(torch.float32)
    else:
        raise ValueError(mode)
    return q.to(v.dtype)


class _Ctx:
    def __init__(self, p, n_blocks, arith, rounding, skip, shared_t):
        if skip is not None and skip not in point_names(n_blocks):
            raise ValueError(f"unknown rounding point {skip!r}")
        self.p, self.nb, self.L, self.dt, self.rounding, self.skip, self.shared_t = p, n_blocks, 1 + 2 * n_blocks, arith, rounding, skip, shared_t
        self._w = {}
        self.stores = {}             # name -> list of [B, *] tensors as stored (weights excepted): what `flip_free` compares

    def r(self, v, name):
        q = v if (self.rounding is None or name == self.skip) else round_bf16(v, self.rounding)
        if name != "w":
            self.stores.setdefault(name, []).append(q)
        return q

    def W(self, name, time_branch=False):
        """A GEMM weight matrix as the kernels read it: bf16, except the time branch of the shared-t path (fp32 copies)."""
        w = self._w.get(name)
        if w is None:
            w = self.p[name + ".weight"].to(self.dt)
            if not (time_branch and self.shared_t):
                w = self.r(w, "w")
            self._w[name] = w
        return w

    def b(self, name):
        return self.p[name + ".bias"].to(self.dt)

    def layer_names(self, l):
        """(dense, gnorm) of GroupNorm layer l: 0 = pre, then dense1 / dense2 of each block."""
        if l == 0:
            return "pre_dense", "pre_gnorm"
        k, j = (l + 1) // 2, 2 - (l % 2)
        return f"b{k}_dense{j}", f"b{k}_gnorm{j}"


def _silu(a):
    return a * torch.sigmoid(a)


def _dsilu(a):
    s = torch.sigmoid(a)
    return s * (1.0 + a * (1.0 - s))            # the form of dsilu_f (common.h)


def _embedding(labels, dim, dt, exact_arg=False, revolutions=False):
    """get_timestep_embedding (model.py:37-51).  The argument label * f_k is an fp32 product in the reference (``timesteps.float()[:, None] *
    emb[None, :]``) and in the kernels (temb_from_freq): at label * f up to 999 rad its rounding is 3e-5 rad, two orders above fp32
    arithmetic noise, so the product belongs to the function and not to the arithmetic under test.  sin / cos of it stay exact."""
    half = dim // 2
    freq = torch.exp(torch.arange(half, dtype=torch.float32) * -(math.log(10000) / (half - 1)))
    if exact_arg:
        arg = labels.to(dt)[:, None] * freq.to(dt)[None, :]
    elif revolutions:
        # bf16 storage: v_sin_f32 / v_cos_f32 take the argument in revolutions, rev = arg * (1 / 2 pi) as a second fp32 product
        # (temb_from_freq<FAST>; |rev| <= 159 is inside the instructions' domain).  Subtracting the whole turns is exact in fp32.
        rev = (labels[:, None] * freq[None, :]) * torch.tensor(0.15915494309189535, dtype=torch.float32)
        arg = (rev - torch.round(rev)).to(dt) * (2.0 * math.pi)
    else:
        arg = (labels[:, None] * freq[None, :]).to(dt)
    return torch.cat([torch.sin(arg), torch.cos(arg)], dim=1)


def forward(p, x, labels, *, n_blocks=2, keep=None, drop_p=0.0, shared_t=False, scale_by_sigma=True, arith=torch.float64, rounding="rne",
            skip=None, tape=None):
    """``ScoreModelFC.forward`` as the bf16 kernels evaluate it.  ``x`` [B, D] and ``labels`` [B] (= t * 999) are the fp32 inputs of the call.
    ``keep``: 1 + 2 n_blocks {0, 1} masks [B, H] (train form; dropout as EpiGN<__bf16, true> applies it: SiLU / (1 - p), then the keep
    decision, then the residual).  ``shared_t``: the time branch as ``build_time_table`` forms it (nothing rounded; the labels of the batch
    are then all equal, but nothing here relies on it).  ``tape``: a dict that receives what ``backward`` needs."""
    c = _Ctx(p, n_blocks, arith, rounding, skip, shared_t)
    dt = arith
    labels = labels.to(torch.float32)
    emb = _embedding(labels, p["shared_time_embed.0.weight"].shape[0], dt, exact_arg=(rounding is None or skip == "arg"),
                     revolutions=(not shared_t and skip != "rev"))
    if not shared_t:
        emb = c.r(emb, "emb")
    u = emb @ c.W("shared_time_embed.0", True).t() + c.b("shared_time_embed.0")
    temb = _silu(u)
    if not shared_t:
        temb = c.r(temb, "temb")
    xin = c.r(x.to(dt), "xin")
    hs, xhats, rstds = [], [], []
    for l in range(c.L):
        dense, gn = c.layer_names(l)
        inp = xin if l == 0 else hs[l - 1]
        # K-concat(h, temb) with the packed bias b + b_t (k_bias_cat) / x-path GEMM + the fp32 time-bias row
        a = inp @ c.W(dense).t() + temb @ c.W(dense + "_t", True).t() + (c.b(dense) + c.b(dense + "_t"))
        B = a.shape[0]
        ag = a.reshape(B, 32, H // 32)
        cen = ag - ag.mean(dim=2, keepdim=True)
        rstd = 1.0 / torch.sqrt((cen * cen).mean(dim=2, keepdim=True) + 1e-5)
        xhat = (cen * rstd).reshape(B, H)
        y = _silu(xhat * p[gn + ".weight"].to(dt) + p[gn + ".bias"].to(dt))
        if keep is not None:
            y = y / (1.0 - drop_p) * keep[l].to(dt)
        if l >= 2 and l % 2 == 0:
            y = y + hs[l - 2]
        hs.append(c.r(y, f"h{l}"))
        xhats.append(xhat)
        rstds.append(rstd)
    res = hs[-1] @ c.W("post_dense").t() + c.b("post_dense")
    usig = p["sigmas"].to(dt)[labels.long().clamp(0, p["sigmas"].numel() - 1)] if scale_by_sigma else torch.ones(x.shape[0], dtype=dt)
    if tape is not None:
        tape.update(ctx=c, stores=c.stores, xin=xin, emb=emb, u=u, temb=temb, hs=hs, xhats=xhats, rstds=rstds, usig=usig, keep=keep, drop_p=drop_p)
    return res / usig[:, None]


def backward(tape, g, *, se_bias_stored=True, per_row=None):
    """Hand-written backward of ``forward`` (per-sample-t path) for an upstream gradient ``g`` [B, D] on the network output, as
    ``dposer_scorefc_backward`` computes it: returns (dx, {parameter name: gradient}).  Uses the stored, rounded quantities the kernels
    use (bf16 x_hat, dy, carry, dres, u, dU and the bf16 GEMM operands).  ``se_bias_stored``: the bias gradient of shared_time_embed
    is the column sum of the STORED dU (k_silu_bwd_reduce: sample-major weight gradients and at most 2048 padded samples) or of the
    fp32 values before the store (EpiSiLUBwd: every other case).  ``per_row``: a dict that receives, for the 1-D gradients of the GroupNorm
    layers, the [B, H] terms whose column sums they are."""
    c = tape["ctx"]
    if c.shared_t:
        raise ValueError("the shared-t entry points are forward-only")
    dt, L, p = c.dt, c.L, c.p
    for n in BACKWARD_POINTS:
        c.stores.pop(n, None)                                                # (a tape may be differentiated more than once)
    keep, scale = tape["keep"], (1.0 / (1.0 - tape["drop_p"]) if tape["keep"] is not None else 1.0)
    grads = {}
    dres = c.r(g.to(dt) / tape["usig"][:, None], "dres")
    grads["post_dense.bias"] = dres.sum(0)                                   # k_colsum over the stored dres
    grads["post_dense.weight"] = dres.t() @ tape["hs"][L - 1]
    G = dres @ c.W("post_dense")
    temb = tape["temb"]
    carry, dys = None, [None] * L
    for j in range(L - 1, -1, -1):
        dense, gn = c.layer_names(j)
        even = j % 2 == 0
        gj = G + carry if (even and j < L - 1) else G                        # EpiGNBwd: acc + carry_in
        if even and j >= 2:
            carry = c.r(gj, "carry")                                         # carry_out = g, stored before anything else
        xh = c.r(tape["xhats"][j], "xhat")
        gamma, beta = p[gn + ".weight"].to(dt), p[gn + ".bias"].to(dt)
        da = (gj * keep[j].to(dt) if keep is not None else gj) * _dsilu(gamma * xh + beta)
        grads[gn + ".weight"] = (da * xh).sum(0) * scale
        grads[gn + ".bias"] = da.sum(0) * scale
        if per_row is not None:
            per_row[gn + ".weight"], per_row[gn + ".bias"] = da * xh * scale, da * scale
        dx = da * (gamma * scale)
        B = dx.shape[0]
        m1 = dx.reshape(B, 32, -1).mean(dim=2, keepdim=True)
        m2 = (dx * xh).reshape(B, 32, -1).mean(dim=2, keepdim=True)
        dyf = (tape["rstds"][j] * ((dx.reshape(B, 32, -1) - m1) - xh.reshape(B, 32, -1) * m2)).reshape(B, H)
        grads[dense + ".bias"] = dyf.sum(0)                                  # summed before the store
        grads[dense + "_t.bias"] = grads[dense + ".bias"]
        if per_row is not None:
            per_row[dense + ".bias"] = per_row[dense + "_t.bias"] = dyf
        dy = dys[j] = c.r(dyf, "dy")
        grads[dense + ".weight"] = dy.t() @ (tape["xin"] if j == 0 else tape["hs"][j - 1])
        grads[dense + "_t.weight"] = dy.t() @ temb
        G = dy @ c.W(dense)
    dx_in = G                                                                # fp32 row-major output of the last dgrad
    dtemb = sum(dys[l] @ c.W(c.layer_names(l)[0] + "_t") for l in range(L))
    dUf = dtemb * _dsilu(c.r(tape["u"], "upre"))
    dU = c.r(dUf, "dU")
    grads["shared_time_embed.0.bias"] = (dU if se_bias_stored else dUf).sum(0)
    grads["shared_time_embed.0.weight"] = dU.t() @ tape["emb"]
    for n in ("pre_dense_cond.weight", "pre_dense_cond.bias"):
        grads[n] = torch.zeros_like(p[n], dtype=dt)                          # never used in forward (model.py:111)
    return dx_in, grads


# ---- the shared-t entry points: one Euler-Maruyama step and the prior loss (sub-VP, continuous) -------------------------------------
def _shared_labels(t, B):
    return torch.full((B,), t, dtype=torch.float32) * 999                   # utils.py:152: one fp32 product, the bits of the kernels' label


def em_step(p, x, t, z, *, n_blocks, N=1000, **kw):
    """EulerMaruyamaPredictor.update_fn at a shared time ``t`` with injected noise (k_em_update): returns (x_new, x_mean)."""
    dt = kw.get("arith", torch.float64)
    sde = R.SubVP(N=N)
    tv = torch.full((x.shape[0],), float(np.float32(t)), dtype=dt)
    out = forward(p, x, _shared_labels(t, x.shape[0]), n_blocks=n_blocks, shared_t=True, **kw)
    score = -out / sde.marginal_prob(torch.zeros_like(out), tv)[1][:, None]
    drift, g = sde.sde(x.to(dt), tv)
    drift = drift - g[:, None] ** 2 * score
    x_mean = x.to(dt) + drift * (-1.0 / N)
    return x_mean + g[:, None] * math.sqrt(1.0 / N) * z.to(dt), x_mean


def prior_grad(p, x0, t, z, *, weighted, n_blocks, **kw):
    """``dposer_prior_loss`` with reduction 'mean': returns (loss, d loss / d x0 = 2 w (x0 - x0_hat) / n).  x_t is formed in the
    arithmetic under test (fp32 in k_perturb_shared), stored in bf16 for the network and kept in fp32 for the Tweedie estimate."""
    dt = kw.get("arith", torch.float64)
    sde = R.SubVP()
    tv = torch.full((x0.shape[0],), float(np.float32(t)), dtype=dt)
    mean, std = sde.marginal_prob(x0.to(dt), tv)
    x_t = mean + std[:, None] * z.to(dt)
    out = forward(p, x_t, _shared_labels(t, x0.shape[0]), n_blocks=n_blocks, shared_t=True, **kw)
    score = -out / std[:, None]
    alpha, sigma = sde.alpha_sigma(tv)
    x0_hat = (x_t + (sigma ** 2)[:, None] * score) / alpha
    snr = alpha / torch.sqrt(sigma ** 2)[:, None]
    w = 0.5 * torch.sqrt(1 + snr) if weighted else torch.full_like(snr, 0.5)
    diff = x0.to(dt) - x0_hat
    n = x0.numel()
    return (w * diff ** 2).sum() / n, 2 * w * diff / n


# ---- the row rule ------------------------------------------------------------------------------------------------------------------
# Reference alone.  A flip of a store is an exact event there: a row of the float32-arithmetic oracle is *flip-free* when every value it
# stored (at every rounding point) has the bits the float64-arithmetic oracle stored.  e_ref is the largest error of a flip-free row --
# fp32 arithmetic and nothing else.  A flip need not be consequential: bf16 is a floating-point format, the ulp of a small element is small,
# and a flipped sin(.) ~ 1e-3 of the embedding moves the output by less than the arithmetic does.  So rows are classed by their error, on
# the reference exactly as on the GPU: clean <=> error <= tau = 8 e_ref.
TAU_FACTOR = 8.0


def row_err(got, want):
    got, want = torch.as_tensor(got).double(), torch.as_tensor(want).double()
    return ((got - want).norm(dim=1) / want.norm(dim=1).clamp_min(1e-300)).numpy()


def elem_err(got, want):
    """Element-wise error in the normalisation of rule (e): |got - want| / (|want| + RMS of the row of want)."""
    got, want = torch.as_tensor(got).double(), torch.as_tensor(want).double()
    return (got - want).abs() / (want.abs() + want.pow(2).mean(dim=1, keepdim=True).sqrt())


def coverage(clean):
    """(fewest clean rows in an aligned group of 32 rows, number of row positions mod 32 that occur among the clean rows)."""
    clean = np.asarray(clean, dtype=bool)
    groups = [int(clean[i:i + 32].sum()) for i in range(0, len(clean), 32)]
    return min(groups), len(set(np.nonzero(clean)[0] % 32))


def flip_free(s32, s64, exclude=()):
    """Rows whose stores agree bit for bit between two runs of the oracle (dicts name -> list of [B, *] tensors)."""
    ok = None
    for name, lst in s64.items():
        if name in exclude:
            continue
        for a, b in zip(s32[name], lst):
            m = (a.double() == b.double()).reshape(a.shape[0], -1).all(dim=1)
            ok = m if ok is None else ok & m
    return ok.numpy()


def row_stats(q32, q64, plain64, ff):
    """The per-case record of one compared tensor, float32-arithmetic oracle against the float64-arithmetic one: share of flip-free rows,
    e_ref (their largest error) and el_ref (their largest element-wise error, ``elem_err``), clean share p_ref (error <= 8 e_ref), f_ref (smallest error of a non-clean row), the share of rows in
    the band (8 e_ref, 16 e_ref] (the rows that keep f_ref below 16 e_ref), d_max (largest per-row designed error: faithful against plain
    float64 oracle) and the coverage of the clean rows."""
    e = row_err(q32, q64)
    e_ref = float(e[ff].max())
    tau = TAU_FACTOR * e_ref
    clean = e <= tau
    gmin, npos = coverage(clean)
    return dict(flip_free=float(ff.mean()), e_ref=e_ref, el_ref=float(elem_err(q32, q64)[torch.as_tensor(ff)].max()), p_ref=float(clean.mean()), f_ref=float(e[~clean].min()) if (~clean).any() else float("inf"),
                band=float(((e > tau) & (e <= 2 * tau)).mean()), d_max=float(row_err(q64, plain64).max()), group_min=gmin, positions=npos)


def check_rows(got, want, rec, log=None):
    """The row rule of the GPU tests: ``got`` (kernel) against ``want`` (float64-arithmetic faithful oracle), bounds from ``rec``.
    Returns the clean-row mask.  tau = 8 e_ref: MFMA summation order and the three 1-ulp hardware transcendentals (v_exp, v_rcp, v_rsq)
    that the CPU reference does not have.
    (e) is held to 8 el_ref, the same construction element by element (el_ref: the largest ``elem_err`` of a flip-free reference row,
    about 4 e_ref), not to tau: a clean row may carry a flip of a small element, which puts its whole error (< tau in the row norm)
    into a few outputs -- the float32-arithmetic oracle itself has clean rows at 2.5 tau element-wise (4.6e-6 at B = 2304), and so has
    the GPU (4.4e-6)."""
    got, want = torch.as_tensor(got).double().cpu(), torch.as_tensor(want).double()
    tau = TAU_FACTOR * rec["e_ref"]
    e = row_err(got, want)
    clean = e <= tau
    share = float(clean.mean())
    worst_clean = float(e[clean].max()) if clean.any() else float("nan")
    worst_flipped = float(e[~clean].max()) if (~clean).any() else 0.0
    if log is not None:
        log("clean_share", share)
        log("max_clean_row_err", worst_clean)
        log("max_flipped_row_err", worst_flipped)
    print(f"rows {len(e)}: clean share {share:.3f} (p_ref {rec['p_ref']:.3f}), largest clean row {worst_clean:.2e} (tau {tau:.2e}), "
          f"largest flipped row {worst_flipped:.2e} (3 d_max {3 * rec['d_max']:.2e}), smallest flipped row "
          f"{float(e[~clean].min()) if (~clean).any() else float('inf'):.2e}")
    assert worst_flipped <= 3.0 * rec["d_max"], ("(a) a non-clean row lies beyond 3 d_max: a flipped row is a second draw of the same "
                                                 "rounding noise", worst_flipped, rec["d_max"])
    assert share >= rec["p_ref"] ** 3, ("(b) clean share below p_ref^3 (flips are Poisson in the noise amplitude; the kernel is granted "
                                        "three times the reference's)", share, rec["p_ref"])
    gmin, npos = coverage(clean)
    assert gmin >= 1, "(c) an aligned group of 32 rows has no clean row"
    assert npos == min(32, len(e)), ("(d) a row position mod 32 does not occur among the clean rows", npos)
    el = elem_err(got, want)[torch.as_tensor(clean)]
    worst_el = float(el.max()) if el.numel() else 0.0
    tau_el = TAU_FACTOR * rec["el_ref"]
    print(f"largest element-wise error on a clean row {worst_el:.2e} (8 el_ref {tau_el:.2e})")
    if log is not None:
        log("max_clean_elem_err", worst_el)
    assert worst_el <= tau_el, ("(e) element-wise error on a clean row above 8 el_ref (|want| + row RMS)", worst_el, tau_el)
    return clean


# ---- cases -------------------------------------------------------------------------------------------------------------------------
def case_weights(seed, D, n_blocks):
    """Deterministic weights of a case: tests/golden/weights.py at ``seed`` with every tensor perturbed by 0.05 N(0, 1), as
    test_other_model_configurations_vs_oracle perturbs the default initialisation (every bias / gain matters)."""
    from weights import make_weights
    w = make_weights(seed, D=D, n_blocks=n_blocks)
    rs = np.random.RandomState(1000 + seed)
    for k in w:
        w[k] = w[k] + torch.tensor((0.05 * rs.standard_normal(tuple(w[k].shape))).astype(np.float32))
    w["sigmas"] = R.sigma_table()
    return w


def case_inputs(seed, B, D):
    """x, t in [1e-3, 1), the upstream gradient / noise g: fp32, from one numpy stream."""
    rs = np.random.RandomState(seed)
    x = torch.tensor(rs.standard_normal((B, D)).astype(np.float32))
    t = torch.tensor(rs.uniform(1e-3, 1.0, B).astype(np.float32))
    g = torch.tensor(rs.standard_normal((B, D)).astype(np.float32))
    return x, t, g


# name: kind, B, D, n_blocks, weight seed, input seed, (+ what the kind needs).  The tiling switches of a case live in the GPU test.
# Input seeds: the first seed from 0 at which the case meets `unmet_conditions` (where it is not 0, a row of seed 0 lay in (8, 16] e_ref).
CASES = {
    # forward, eval, per-sample t: one batch per tiling of main_shape / gn_shape / final_shape
    "fwd_b160": dict(kind="fwd", B=160, D=63, nb=1, wseed=3, seed=0),          # 192 padded samples, 128x32 (stands in for B = 1: see test_gpu_bf16_faithful.py)
    "fwd_b200": dict(kind="fwd", B=200, D=63, nb=1, wseed=3, seed=7),          # 256 padded samples, 128x32
    "fwd_b1000": dict(kind="fwd", B=1000, D=63, nb=1, wseed=3, seed=0),        # 1024, 128x32
    "fwd_b1100": dict(kind="fwd", B=1100, D=63, nb=1, wseed=3, seed=0),        # 1280, SHAPE_SMALL64
    "fwd_b2304": dict(kind="fwd", B=2304, D=63, nb=1, wseed=3, seed=0),        # 2304, 128x128; again with 256x256 forced
    "fwd_b200_d126": dict(kind="fwd", B=200, D=126, nb=1, wseed=4, seed=9),
    "fwd_b1100_d126": dict(kind="fwd", B=1100, D=126, nb=1, wseed=4, seed=0),  # also over the 64x128 post_dense tiling
    "fwd_b200_2blk": dict(kind="fwd", B=200, D=63, nb=2, wseed=5, seed=10),     # the shipped depth
    "fwd_b2304_2blk": dict(kind="fwd", B=2304, D=63, nb=2, wseed=5, seed=0),
    # forward, train form, in-kernel Philox dropout (keep masks from oracle/philox.py at the model's seed, step 1)
    "drop01_b200": dict(kind="drop", B=200, D=63, nb=1, wseed=6, seed=0, drop_p=0.1),
    "drop05_b200": dict(kind="drop", B=200, D=63, nb=1, wseed=6, seed=1, drop_p=0.5),
    "drop01_b1100": dict(kind="drop", B=1100, D=63, nb=1, wseed=6, seed=0, drop_p=0.1),
    "drop05_b1100": dict(kind="drop", B=1100, D=63, nb=1, wseed=6, seed=0, drop_p=0.5),
    # shared t: one Euler-Maruyama step (loop index `step` of N = 1000) and the prior loss at two times
    "em_b300": dict(kind="em", B=300, D=63, nb=1, wseed=7, seed=0, step=10),
    "em_b1100": dict(kind="em", B=1100, D=63, nb=1, wseed=7, seed=0, step=10),
    "prior_b300": dict(kind="prior", B=300, D=63, nb=1, wseed=7, seed=0, ts=(0.31, 0.77)),
    "prior_b1100": dict(kind="prior", B=1100, D=63, nb=1, wseed=7, seed=0, ts=(0.31, 0.77)),
    # autograd: out and x.grad
    "autograd_b400": dict(kind="grad", B=400, D=63, nb=1, wseed=8, seed=0),
    "autograd_b1100": dict(kind="grad", B=1100, D=63, nb=1, wseed=8, seed=1),
    # parameter gradients, two passes
    "wgrad_b512": dict(kind="wgrad", B=512, D=63, nb=1, wseed=8, seed=0),
    "wgrad_b1100": dict(kind="wgrad", B=1100, D=63, nb=1, wseed=8, seed=0),
    "wgrad_b2304": dict(kind="wgrad", B=2304, D=63, nb=1, wseed=8, seed=0, se_bias_stored=False),   # > 2048 padded samples: EpiSiLUBwd
    "wgrad_b512_tr0": dict(kind="wgrad", B=512, D=63, nb=1, wseed=8, seed=0, se_bias_stored=False),  # DPOSER_WGRAD_TR=0: EpiSiLUBwd
}
DROPOUT_RNG_SEED, DROPOUT_RNG_STEP = 12345, 1      # ScoreModelFC._rng_seed at config seed 0 and the step of the first training forward


def dropout_masks(case):
    from oracle import philox as PH
    c = CASES[case]
    return [torch.tensor(PH.dropout_keep_mask(c["B"], H, site, DROPOUT_RNG_STEP, DROPOUT_RNG_SEED, c["drop_p"])) for site in range(1 + 2 * c["nb"])]


def em_time(step, N=1000, eps=1e-3):
    return float(torch.linspace(1.0, eps, N)[step])


def tile_err(got, want):
    """Largest error of an aligned 32 x 32 tile of a matrix: tile error (L2) over the tile's RMS-based norm, floored at the tensor RMS."""
    got, want = torch.as_tensor(got).double(), torch.as_tensor(want).double()
    R_, C_ = want.shape
    pr, pc = (-R_) % 32, (-C_) % 32
    pad = lambda a: torch.nn.functional.pad(a, (0, pc, 0, pr)).reshape((R_ + pr) // 32, 32, (C_ + pc) // 32, 32)
    err = pad(got - want).pow(2).sum(dim=(1, 3)).sqrt()
    cnt = pad(torch.ones_like(want)).sum(dim=(1, 3))
    rms_t = (pad(want).pow(2).sum(dim=(1, 3)) / cnt).sqrt()
    rms = torch.maximum(rms_t, want.pow(2).mean().sqrt())
    return float((err / (rms * cnt.sqrt())).max())


@functools.lru_cache(maxsize=None)
def reference(case, arith=torch.float64, rounding="rne"):
    """What the oracle yields for a case in one arithmetic (cached: shared by the tests of a session, never modified).  A dict: the
    compared tensors by name ('out', 'dx', 'grad_<i>', ...), 'stores_<name>' = the stores that tensor depends on (for ``flip_free``),
    and for the differentiated kinds 'tape' and 'grads'.  ``rounding=None``: the plain oracle (compared tensors only)."""
    c = CASES[case]
    p = case_weights(c["wseed"], c["D"], c["nb"])
    x, t, g = case_inputs(c["seed"], c["B"], c["D"])
    kw = dict(n_blocks=c["nb"], arith=arith, rounding=rounding)
    kind = c["kind"]
    if kind in ("fwd", "drop"):
        tape = {}
        extra = dict(keep=dropout_masks(case), drop_p=c["drop_p"]) if kind == "drop" else {}
        return dict(out=forward(p, x, t * 999, tape=tape, **extra, **kw), stores_out=tape["stores"])
    if kind == "em":
        tape = {}
        xn, xm = em_step(p, x, em_time(c["step"]), g, tape=tape, **kw)
        return dict(out=xm, x_new=xn, stores_out=tape["stores"])
    if kind == "prior":
        o = {}
        for i, tt in enumerate(c["ts"]):
            tape = {}
            o[f"loss_{i}"], o[f"grad_{i}"] = prior_grad(p, x, tt, g, weighted=(i == 0), tape=tape, **kw)
            o[f"stores_grad_{i}"] = tape["stores"]
        return o
    tape = {}
    out = forward(p, x, t * 999, tape=tape, **kw)
    fwd_stores = {k: list(v) for k, v in tape["stores"].items()}
    dx, grads = backward(tape, g, se_bias_stored=c.get("se_bias_stored", True))
    if rounding is None:
        return dict(out=out, dx=dx)
    return dict(out=out, dx=dx, tape=tape if kind == "wgrad" else None, grads=grads, stores_out=fwd_stores,
                stores_dx={k: list(v) for k, v in tape["stores"].items() if k not in ("upre", "dU")})      # (dx does not depend on the time-branch dgrad)


def compared(case):
    """Names of the tensors of a case that the row rule is applied to."""
    kind = CASES[case]["kind"]
    if kind == "prior":
        return tuple(f"grad_{i}" for i in range(len(CASES[case]["ts"])))
    return ("out", "dx") if kind in ("grad", "wgrad") else ("out",)


def masked_param_grads(case, S, arith=torch.float64):
    """Pass 2 of the parameter-gradient test on the reference: the backward with ``g`` zeroed outside the rows ``S`` (bool mask)."""
    c = CASES[case]
    ref = reference(case, arith)
    _, _, g = case_inputs(c["seed"], c["B"], c["D"])
    g = g * torch.as_tensor(np.asarray(S), dtype=g.dtype)[:, None]
    return backward(ref["tape"], g, se_bias_stored=c.get("se_bias_stored", True))


def reference_clean_rows(case, name):
    """Rows of the float32-arithmetic oracle that are clean against the float64-arithmetic one (error <= 8 e_ref of the record)."""
    return row_err(reference(case, torch.float32)[name], reference(case)[name]) <= TAU_FACTOR * RECORD[case][name]["e_ref"]


def param_grad_errors(case, S):
    """Float32-arithmetic against float64-arithmetic oracle for the parameter gradients of the sum over the rows S: per tensor the rel-L2
    error and, for matrices, ``tile_err``.  S must be clean on the reference (nothing rounded differs: fp32 accumulation is what is left)."""
    _, g64 = masked_param_grads(case, S)
    _, g32 = masked_param_grads(case, S, torch.float32)
    rel, tile = {}, {}
    for n, w in g64.items():
        if n.startswith("pre_dense_cond"):
            continue
        rel[n] = float((g32[n].double() - w).norm() / w.norm())
        if w.dim() == 2:
            tile[n] = tile_err(g32[n], w)
    return rel, tile


def is_layer_vector(name):
    """The 1-D gradients of the GroupNorm layers: gamma, beta and the two biases of every layer."""
    return "gnorm" in name or (name.endswith(".bias") and "dense" in name and not name.startswith(("post_dense", "pre_dense_cond")))


def param_grad_bounds(case, S):
    """Bounds of the parameter-gradient test: 8 x ``param_grad_errors`` -- per tensor (and per tile) for the matrices, post_dense.bias and
    shared_time_embed.0.bias; for the 1-D gradients of the GroupNorm layers 8 x the LARGEST reference error among them.
    Why pooled: S holds the rows that are clean in out and x.grad, which is all a caller can see.  A flip of the stored x_hat moves
    dy by less than half a bf16 ulp about every second time; dy is then stored with the same bits, x.grad does not change and the row
    stays in S -- but gamma / beta / bias gradients are sums of the fp32 values BEFORE that store, and the batch sum is dominated by the
    few rows with small sigma(t).  One such row puts 4e-6 ... 1e-5 into whichever layer it happens in, against 2e-7 ... 7e-7 without:
    between two float32 realisations of this oracle on the CPU (another summation order in the matrix products) the error of a single
    such tensor differs by 0.02x ... 41x, the largest over the group by 0.5x ... 1.7x (six runs at B = 512 and 1100)."""
    rel, tile = param_grad_errors(case, S)
    pooled = max(v for n, v in rel.items() if is_layer_vector(n))
    return {n: 8 * (pooled if is_layer_vector(n) else v) for n, v in rel.items()}, {n: 8 * v for n, v in tile.items()}


def regenerate(case):
    """The per-case record from the reference alone: ``row_stats`` of every compared tensor; for the parameter-gradient cases also the
    number of rows S that are clean in both out and dx on the reference and ``param_grad_errors`` over them."""
    r64, r32, pl = reference(case), reference(case, torch.float32), reference(case, torch.float64, None)
    rec = {}
    for n in compared(case):
        rec[n] = row_stats(r32[n], r64[n], pl[n], flip_free(r32["stores_" + n], r64["stores_" + n]))
    if CASES[case]["kind"] == "wgrad":
        S = np.ones(CASES[case]["B"], dtype=bool)
        for n in compared(case):
            S &= row_err(r32[n], r64[n]) <= TAU_FACTOR * rec[n]["e_ref"]
        rec["S"] = int(S.sum())
        rec["rel"], rec["tile"] = param_grad_errors(case, S)
    return rec


GAP_MAX_B = 200      # up to this batch the input seed is chosen so that no reference row lies in (8 e_ref, 16 e_ref]
BAND_MAX = 0.05      # larger batches: at most this share of rows there (measured <= 0.024; see unmet_conditions)
S_MIN = 64


def unmet_conditions(case, rec):
    """The conditions a case must meet on the reference alone before a GPU sees it; returns what is not met (empty: all met).
    * p_ref >= 0.5; every aligned group of 32 rows holds >= 4 clean rows; every row position mod 32 occurs among the clean rows.
    * The split is real: f_ref >= 16 e_ref, i.e. tau = 8 e_ref lies a factor two below the nearest non-clean row.  A flip of a small
      element is a small error, so flipped rows form a thin continuum down to the arithmetic level (about 1 % of the rows per factor two
      between 1e-6 and 1e-4) and a batch of B rows has about B / 100 of them in (8, 16] e_ref: up to GAP_MAX_B rows the input seed is
      chosen so that there is none; above it no seed can, and the condition is that at most BAND_MAX of the rows lie there (they are
      non-clean rows like any other for the GPU rule, bounded by (a); they cost the clean share at most that much, an order below the
      slack p_ref - p_ref^3 >= 0.375 that (b) grants).
    * parameter-gradient cases: at least S_MIN rows are clean in both out and dx."""
    bad = []
    for n in compared(case):
        r = rec[n]
        if not r["p_ref"] >= 0.5:
            bad.append(f"{n}: p_ref {r['p_ref']:.3f} < 0.5")
        if r["group_min"] < 4:
            bad.append(f"{n}: an aligned group of 32 rows holds {r['group_min']} clean rows")
        if r["positions"] != 32:
            bad.append(f"{n}: {r['positions']} of 32 row positions occur among the clean rows")
        if CASES[case]["B"] <= GAP_MAX_B:
            if not r["f_ref"] >= 16 * r["e_ref"]:
                bad.append(f"{n}: f_ref {r['f_ref']:.2e} < 16 e_ref = {16 * r['e_ref']:.2e}")
        elif r["band"] > BAND_MAX:
            bad.append(f"{n}: {r['band']:.3f} of the rows lie in (8, 16] e_ref")
    if CASES[case]["kind"] == "wgrad" and rec["S"] < S_MIN:
        bad.append(f"|S| = {rec['S']} < {S_MIN}")
    return bad


# regenerate() of every case (`python tests/bf16_ref.py` prints this dict); test_bf16_ref_cpu.py checks it against a fresh regeneration and
# asserts the conditions on it, the GPU tests read their bounds from it.
RECORD = {
    "fwd_b160": {"out": dict(flip_free=0.675, e_ref=2.126e-07, el_ref=4.855e-07, p_ref=0.8812, f_ref=4.399e-06, band=0, d_max=0.006563, group_min=27, positions=32)},
    "fwd_b200": {"out": dict(flip_free=0.575, e_ref=2.195e-07, el_ref=7.072e-07, p_ref=0.825, f_ref=3.019e-05, band=0, d_max=0.006764, group_min=8, positions=32)},
    "fwd_b1000": {"out": dict(flip_free=0.625, e_ref=2.294e-07, el_ref=1.209e-06, p_ref=0.843, f_ref=1.850e-06, band=0.012, d_max=0.006584, group_min=4, positions=32)},
    "fwd_b1100": {"out": dict(flip_free=0.6045, e_ref=2.473e-07, el_ref=8.995e-07, p_ref=0.8236, f_ref=2.005e-06, band=0.006364, d_max=0.007507, group_min=9, positions=32)},
    "fwd_b2304": {"out": dict(flip_free=0.6128, e_ref=2.286e-07, el_ref=1.042e-06, p_ref=0.8273, f_ref=1.829e-06, band=0.008681, d_max=0.006807, group_min=21, positions=32)},
    "fwd_b200_d126": {"out": dict(flip_free=0.61, e_ref=1.540e-07, el_ref=5.211e-07, p_ref=0.845, f_ref=3.259e-06, band=0, d_max=0.005639, group_min=6, positions=32)},
    "fwd_b1100_d126": {"out": dict(flip_free=0.6191, e_ref=2.178e-07, el_ref=9.807e-07, p_ref=0.8145, f_ref=1.829e-06, band=0.008182, d_max=0.005562, group_min=9, positions=32)},
    "fwd_b200_2blk": {"out": dict(flip_free=0.475, e_ref=2.033e-07, el_ref=4.628e-07, p_ref=0.775, f_ref=6.994e-06, band=0, d_max=0.006264, group_min=7, positions=32)},
    "fwd_b2304_2blk": {"out": dict(flip_free=0.4783, e_ref=2.015e-07, el_ref=7.100e-07, p_ref=0.7522, f_ref=1.644e-06, band=0.007378, d_max=0.006266, group_min=19, positions=32)},
    "drop01_b200": {"out": dict(flip_free=0.59, e_ref=2.524e-07, el_ref=8.111e-07, p_ref=0.86, f_ref=5.244e-06, band=0, d_max=0.005709, group_min=8, positions=32)},
    "drop05_b200": {"out": dict(flip_free=0.805, e_ref=1.757e-07, el_ref=5.361e-07, p_ref=0.905, f_ref=6.187e-06, band=0, d_max=0.006952, group_min=8, positions=32)},
    "drop01_b1100": {"out": dict(flip_free=0.6755, e_ref=2.361e-07, el_ref=8.196e-07, p_ref=0.8555, f_ref=1.943e-06, band=0.01091, d_max=0.00679, group_min=10, positions=32)},
    "drop05_b1100": {"out": dict(flip_free=0.7855, e_ref=2.150e-07, el_ref=6.912e-07, p_ref=0.9127, f_ref=1.797e-06, band=0.006364, d_max=0.006918, group_min=12, positions=32)},
    "em_b300": {"out": dict(flip_free=0.3467, e_ref=2.081e-07, el_ref=5.771e-07, p_ref=0.6733, f_ref=1.723e-06, band=0.01, d_max=0.004727, group_min=7, positions=32)},
    "em_b1100": {"out": dict(flip_free=0.3991, e_ref=2.446e-07, el_ref=6.032e-07, p_ref=0.7182, f_ref=2.146e-06, band=0.01545, d_max=0.004727, group_min=9, positions=32)},
    "prior_b300": {"grad_0": dict(flip_free=0.4433, e_ref=1.413e-07, el_ref=3.099e-07, p_ref=0.7333, f_ref=1.590e-06, band=0.01333, d_max=0.002092, group_min=9, positions=32),
                  "grad_1": dict(flip_free=0.3967, e_ref=2.210e-07, el_ref=4.972e-07, p_ref=0.7233, f_ref=1.826e-06, band=0.006667, d_max=0.005137, group_min=11, positions=32)},
    "prior_b1100": {"grad_0": dict(flip_free=0.4082, e_ref=1.576e-07, el_ref=4.230e-07, p_ref=0.7118, f_ref=1.483e-06, band=0.01636, d_max=0.0022, group_min=9, positions=32),
                   "grad_1": dict(flip_free=0.38, e_ref=2.460e-07, el_ref=6.370e-07, p_ref=0.7009, f_ref=1.971e-06, band=0.01636, d_max=0.005096, group_min=9, positions=32)},
    "autograd_b400": {"out": dict(flip_free=0.6575, e_ref=2.404e-07, el_ref=7.595e-07, p_ref=0.8525, f_ref=4.427e-06, band=0, d_max=0.006517, group_min=11, positions=32),
                     "dx": dict(flip_free=0.2625, e_ref=1.953e-07, el_ref=5.827e-07, p_ref=0.6875, f_ref=1.726e-06, band=0.0075, d_max=0.00854, group_min=11, positions=32)},
    "autograd_b1100": {"out": dict(flip_free=0.6355, e_ref=2.384e-07, el_ref=7.667e-07, p_ref=0.8545, f_ref=1.926e-06, band=0.009091, d_max=0.006835, group_min=12, positions=32),
                      "dx": dict(flip_free=0.2445, e_ref=2.563e-07, el_ref=8.579e-07, p_ref=0.6718, f_ref=2.161e-06, band=0.01545, d_max=0.007964, group_min=10, positions=32)},
    "wgrad_b512": {"out": dict(flip_free=0.6211, e_ref=2.197e-07, el_ref=6.558e-07, p_ref=0.8184, f_ref=2.026e-06, band=0.009766, d_max=0.006545, group_min=21, positions=32),
                  "dx": dict(flip_free=0.2539, e_ref=1.775e-07, el_ref=5.808e-07, p_ref=0.6797, f_ref=1.514e-06, band=0.005859, d_max=0.008814, group_min=17, positions=32),
                  "S": 328,
                  "worst_rel": ("shared_time_embed.0.weight", 1.36e-05),
                  "worst_tile": ("shared_time_embed.0.weight", 5.89e-05)},
    "wgrad_b1100": {"out": dict(flip_free=0.6227, e_ref=2.122e-07, el_ref=8.221e-07, p_ref=0.8273, f_ref=1.750e-06, band=0.008182, d_max=0.007259, group_min=8, positions=32),
                   "dx": dict(flip_free=0.22, e_ref=2.525e-07, el_ref=7.376e-07, p_ref=0.6409, f_ref=2.099e-06, band=0.008182, d_max=0.008767, group_min=6, positions=32),
                   "S": 671,
                   "worst_rel": ("shared_time_embed.0.weight", 6.16e-06),
                   "worst_tile": ("shared_time_embed.0.weight", 1.80e-05)},
    "wgrad_b2304": {"out": dict(flip_free=0.6254, e_ref=2.452e-07, el_ref=8.509e-07, p_ref=0.8403, f_ref=1.996e-06, band=0.008247, d_max=0.006821, group_min=22, positions=32),
                   "dx": dict(flip_free=0.2279, e_ref=2.643e-07, el_ref=9.867e-07, p_ref=0.6701, f_ref=2.159e-06, band=0.01302, d_max=0.008603, group_min=15, positions=32),
                   "S": 1463,
                   "worst_rel": ("shared_time_embed.0.weight", 1.04e-05),
                   "worst_tile": ("shared_time_embed.0.weight", 2.93e-05)},
    "wgrad_b512_tr0": {"out": dict(flip_free=0.6211, e_ref=2.197e-07, el_ref=6.558e-07, p_ref=0.8184, f_ref=2.026e-06, band=0.009766, d_max=0.006545, group_min=21, positions=32),
                      "dx": dict(flip_free=0.2539, e_ref=1.775e-07, el_ref=5.808e-07, p_ref=0.6797, f_ref=1.514e-06, band=0.005859, d_max=0.008814, group_min=17, positions=32),
                      "S": 328,
                      "worst_rel": ("shared_time_embed.0.weight", 1.36e-05),
                      "worst_tile": ("shared_time_embed.0.weight", 5.89e-05)},
}


def format_record(rec):
    """``rec`` ({case: regenerate(case)}) as the text of the RECORD literal above (four digits; of the per-tensor parameter-gradient
    errors only the worst: the GPU test forms its bounds with ``param_grad_errors`` over the rows it actually sums)."""
    num = lambda v: repr(v) if isinstance(v, int) else (f"{v:.4g}" if v >= 1e-3 or v == 0 else f"{v:.3e}")
    lines = ["RECORD = {"]
    for k, r in rec.items():
        parts = []
        for n, st in r.items():
            if n in ("rel", "tile"):
                w = max(st, key=st.get)
                parts.append(f'"worst_{n}": ("{w}", {st[w]:.2e})')
            elif n == "S":
                parts.append(f'"S": {st}')
            else:
                parts.append(f'"{n}": dict(' + ", ".join(f"{a}={num(b)}" for a, b in st.items()) + ")")
        lines.append(f'    "{k}": {{' + (",\n" + " " * (8 + len(k))).join(parts) + "},")
    return "\n".join(lines + ["}"])


if __name__ == "__main__":
    import sys
    torch.set_num_threads(8)
    print(format_record({n: regenerate(n) for n in (sys.argv[1:] or list(CASES))}))


