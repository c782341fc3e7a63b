"""The bf16 mode (the default precision, the one bench.py times) against the rounding-faithful float64 oracle of tests/bf16_ref.py.

Every test applies the row rule ``bf16_ref.check_rows``: a row is clean if its relative L2 error against the float64-arithmetic
faithful oracle is <= tau = 8 e_ref (e_ref: the largest error of a flip-free row of the float32-arithmetic oracle, about 2.2e-7);
(a) every other row lies within 3 d_max, (b) the clean share is >= p_ref^3, (c) every aligned group of 32 rows has a clean row,
(d) every row position mod 32 occurs among the clean rows, (e) clean rows agree element-wise to 8 el_ref (|want| + row RMS), el_ref
being e_ref's element-wise counterpart (``check_rows`` says why tau itself cannot bound single elements).  The numbers come from
``bf16_ref.RECORD`` (checked by tests/test_bf16_ref_cpu.py); measured values are logged with DPOSER_LOG_ERR and printed.

Measured over all cases below (bound beside it): tau 1.1e-6 ... 2.1e-6; clean share 0.57 ... 0.91 (p_ref 0.64 ... 0.91, bound p_ref^3 =
0.26 ... 0.76); largest flipped row 7.1e-4 ... 4.1e-3 (3 d_max = 6.3e-3 ... 2.6e-2); largest element-wise error on a clean row
9.9e-7 ... 5.8e-6 (8 el_ref = 2.5e-6 ... 9.7e-6); every aligned group of 32 rows and every row position has clean rows.

B = 1 (64 padded samples) cannot meet (c) / (d): the smallest batch that does, with four rows per position, is B = 160 (``fwd_b160``);
the one-row batch is held to it by bit-identity instead (``test_one_row_batch_carries_the_bits_of_its_row``)."""
import numpy as np
import pytest
import torch

import bf16_ref as Q
import score_plan as SP
from gpu_common import DEV, t2n
from helpers import _log_measured

pytestmark = pytest.mark.gpu
torch.set_num_threads(8)


def _dev(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.float32).to(DEV)


def _model(case, dropout=0.0):
    """ScoreModelFC of a case in bf16 mode: tests/golden/weights.py with every parameter perturbed (``bf16_ref.case_weights``)."""
    from dposer_amd.algorithms.advanced.model import ScoreModelFC
    from dposer_amd.configs import load_config
    c = Q.CASES[case]
    cfg = load_config("configs.subvp.amass_scorefc_continuous.get_config")
    cfg.model.dropout = dropout
    m = ScoreModelFC(cfg, n_poses=21, pose_dim=c["D"] // 21, hidden_dim=Q.H, embed_dim=Q.E, n_blocks=c["nb"])
    sd = m.state_dict()
    for k, v in Q.case_weights(c["wseed"], c["D"], c["nb"]).items():
        if k != "sigmas":
            sd[k] = v
    m.load_state_dict(sd)
    m.precision = "bf16"
    m.to(DEV).eval()
    return m, Q.case_inputs(c["seed"], c["B"], c["D"])


def _force(tuning_env, m, case, env):
    """Load the switches of a case and assert through ``dposer_scorefc_plan`` what they select.  ``score_plan.POLICY_BIG`` / ``POLICY_MID`` put the
    256x256 / 128x128 tilings (and 64x128 for post_dense / dx) onto the small batches of the cases: the faithful oracle and its row rule
    do not depend on the tiling, so the cases and their bounds are reused as they are."""
    tuning_env(**env)
    pl = SP.model_plan(m, Q.CASES[case]["B"])
    if env.get("DPOSER_SMALL_TILE_MAX") == "0":
        tile = SP.BIG if "DPOSER_BIG_MIN_BATCH" in env else SP.MID
        assert (pl.gn, pl.gn_bwd, pl.time, pl.final, pl.wgrad) == (tile, tile, tile, SP.FINAL, tile), pl
        assert pl.wgrad_form == (SP.SPLIT_K if env.get("DPOSER_WGRAD_BATCHED") == "0" else SP.ONE_LAUNCH), pl
    return pl


BIG_SPLITK = dict(SP.POLICY_BIG, DPOSER_WGRAD_BATCHED="0")
MID_SPLITK = dict(SP.POLICY_MID, DPOSER_WGRAD_BATCHED="0")


def _rows(got, case, name):
    return Q.check_rows(t2n(got), Q.reference(case)[name], Q.RECORD[case][name], log=_log_measured)


# ------------------------------------------------------------------------------------------------
# forward, eval, per-sample t
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,env", [
    ("fwd_b160", {}),                                          # 192 padded samples, 128x32
    ("fwd_b200", {}),                                          # 256, 128x32
    ("fwd_b1000", {}),                                         # 1024, 128x32
    ("fwd_b1100", {}),                                         # 1280, SHAPE_SMALL64 (128x64, eight waves: bf16 only)
    ("fwd_b2304", {}),                                         # 2304, 128x128
    ("fwd_b2304", {"DPOSER_BIG_MIN_BATCH": "2304"}),           # 256x256
    ("fwd_b1100", {"DPOSER_FINAL_SMALL_MAX": "0"}),            # post_dense on the 64x128 tiling
    ("fwd_b200_d126", {}), ("fwd_b1100_d126", {}),             # rot6d: D = 126, two 64-channel output blocks
    ("fwd_b200_2blk", {}), ("fwd_b2304_2blk", {}),             # the shipped depth (residual input from layer 2 on)
    ("fwd_b200", SP.POLICY_BIG), ("fwd_b200", SP.POLICY_MID),  # 256 padded samples on one 256x256 tile / two 128x128 tiles, post_dense on 64x128
])
def test_forward_eval_rows_vs_faithful_oracle(case, env, tuning_env):
    m, (x, t, _) = _model(case)
    _force(tuning_env, m, case, env)
    with torch.no_grad():
        out = m(_dev(x), _dev(t) * 999)
    _rows(out, case, "out")      # measured: clean share 0.69 ... 0.83 (p_ref 0.75 ... 0.88), largest flipped row 1.6e-3 ... 3.7e-3


def test_one_row_batch_carries_the_bits_of_its_row():
    """B = 1 (64 padded samples, 63 of them padding): the row rule needs rows at every position, so the one-row call is tied to the
    verified batch instead -- same tiling, same K order: the bits of row 0 of ``fwd_b200``."""
    m, (x, t, _) = _model("fwd_b200")
    with torch.no_grad():
        full = m(_dev(x), _dev(t) * 999)
        one = m(_dev(x[:1]), _dev(t[:1]) * 999)
    assert torch.equal(one, full[:1])


# ------------------------------------------------------------------------------------------------
# forward, train form: in-kernel Philox dropout, 1 / (1 - p) folded into the sigmoid's reciprocal
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,env", [pytest.param(c, {}, id=c) for c in ("drop01_b200", "drop05_b200", "drop01_b1100", "drop05_b1100")] + [
    # the Philox draw of (seed, step, sample, channel) inside the training epilogues of the 256x256 / 128x128 tilings
    pytest.param("drop01_b200", SP.POLICY_BIG, id="drop01_b200-BIG"), pytest.param("drop05_b200", SP.POLICY_BIG, id="drop05_b200-BIG"),
    pytest.param("drop01_b200", SP.POLICY_MID, id="drop01_b200-MID"), pytest.param("drop05_b200", SP.POLICY_MID, id="drop05_b200-MID")])
def test_forward_train_dropout_rows_vs_faithful_oracle(case, env, tuning_env):
    m, (x, t, _) = _model(case, dropout=Q.CASES[case]["drop_p"])
    _force(tuning_env, m, case, env)
    m.train()
    m._rng_seed, m._rng_step = Q.DROPOUT_RNG_SEED, Q.DROPOUT_RNG_STEP - 1      # the forward below draws at (seed, step 1): the oracle's masks
    with torch.no_grad():
        out = m(_dev(x), _dev(t) * 999)
    assert m._rng_step == Q.DROPOUT_RNG_STEP
    _rows(out, case, "out")      # measured: clean share 0.82 ... 0.91 (p_ref 0.86 ... 0.91), largest flipped row 1.9e-3 ... 2.8e-3


# ------------------------------------------------------------------------------------------------
# shared t: the fp32 time-bias table, x-path GEMMs only
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["em_b300", "em_b1100"])
def test_one_euler_maruyama_step_rows_vs_faithful_oracle(case):
    """One step of the one-call sampler from a given state with injected noise (loop index 10 of 1000: t = 0.99, where the score term of
    the drift is of the size of the state): x_mean by the row rule; x = x_mean + g sqrt(-dt) z element-wise."""
    from dposer_amd.algorithms.advanced import sampling, sde_lib
    c = Q.CASES[case]
    m, (x, _, z) = _model(case)
    sde = sde_lib.subVPSDE(0.1, 20.0, 1000)
    ts = torch.linspace(sde.T, 1e-3, sde.N)
    _, xn, xm = sampling.fused_pc_sample(m, sde, _dev(x), ts, predictor=sampling.EulerMaruyamaPredictor, corrector=None, start_step=c["step"],
                                         run_steps=1, noise=_dev(z)[None, None], traj_stride=0)
    ref = Q.reference(case)
    _rows(xm, case, "out")       # measured: clean share 0.59 / 0.64 (p_ref 0.67 / 0.72), largest flipped row 1.7e-3
    xn, xm = t2n(xn).astype(np.float64), t2n(xm).astype(np.float64)
    noise = (ref["x_new"] - ref["out"]).numpy()
    # the fp32 store of x (half an ulp: 2^-24 |x|) and the fp32 scalar g sqrt(-dt) times z (sqrt, exp, two products: <= 6 ulp of the
    # noise term) -- together below 2^-21 (|x| + |noise|)
    err = np.abs((xn - xm) - noise) / (np.abs(xn) + np.abs(noise))
    _log_measured("noise_term_err", float(err.max()))
    assert float(err.max()) <= 2.0 ** -21                                      # measured 1.2e-7


@pytest.mark.parametrize("case", ["prior_b300", "prior_b1100"])
def test_prior_loss_gradient_rows_vs_faithful_oracle(case):
    """``prior_loss`` at t = 0.31 (weighted) and t = 0.77 (unweighted): its gradient 2 w (x0 - x0_hat) / n by the row rule; the loss is the
    sum of w (x0 - x0_hat)^2 / n over the same rows, so it follows from the kernel's own gradient rows to fp32 summation accuracy, and
    from the oracle's to (2 eps + eps^2) with eps = 3 d_max, the bound of rule (a)."""
    from dposer_amd.algorithms.advanced import sde_lib
    from dposer_amd.prior import prior_loss
    c = Q.CASES[case]
    m, (x, _, z) = _model(case)
    sde = sde_lib.subVPSDE(0.1, 20.0, 1000)
    ref = Q.reference(case)
    for i, tt in enumerate(c["ts"]):
        x0 = _dev(x).requires_grad_(True)
        loss = prior_loss(m, sde, x0, tt, weighted=(i == 0), z=_dev(z))
        loss.backward()
        loss = float(loss.detach())
        _rows(x0.grad, case, f"grad_{i}")      # measured: clean share 0.57 ... 0.68 (p_ref 0.70 ... 0.73), largest flipped row 7.1e-4 ... 1.8e-3
        want_loss, want_grad = float(ref[f"loss_{i}"]), ref[f"grad_{i}"]
        n_over_4w = want_loss / float((want_grad ** 2).sum())                 # loss = sum(grad^2) n / (4 w), w a scalar at a shared t
        own = float((x0.grad.double() ** 2).sum()) * n_over_4w
        eps = 3 * Q.RECORD[case][f"grad_{i}"]["d_max"]
        _log_measured("loss_vs_own_grad", abs(loss - own) / own)
        _log_measured("loss_vs_oracle", abs(loss - want_loss) / want_loss)
        assert abs(loss - own) / own <= 2e-6                           # fp32 block sums (32 ulp); measured 1.2e-7
        assert abs(loss - want_loss) / want_loss <= 2 * eps + eps ** 2  # 1.3e-2 / 3.1e-2; measured 5.3e-6


# ------------------------------------------------------------------------------------------------
# autograd path (forward in the training layout + dposer_scorefc_backward)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["autograd_b400", "autograd_b1100"])
def test_autograd_rows_vs_faithful_oracle(case):
    m, (x, t, g) = _model(case)
    xd = _dev(x).requires_grad_(True)
    out = m(xd, _dev(t) * 999)
    out.backward(_dev(g))
    _rows(out, case, "out")      # measured: clean share 0.85 / 0.82 (p_ref 0.85 / 0.86), largest flipped row 2.2e-3 / 3.8e-3
    _rows(xd.grad, case, "dx")   # measured: clean share 0.72 / 0.65 (p_ref 0.69 / 0.67), largest flipped row 3.0e-3 / 3.7e-3


# ------------------------------------------------------------------------------------------------
# parameter gradients, two passes
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,env", [
    ("wgrad_b512", {}), ("wgrad_b1100", {}),                   # the default path: one lane launch for all 256x256 weight-gradient tiles
    ("wgrad_b2304", {"DPOSER_WGRAD_BATCHED": "0", "DPOSER_WGRAD_BIG": "1", "DPOSER_GNBWD_BIG": "1"}),   # split-K 256x256 wgrads, 256x256 EpiGNBwd
    ("wgrad_b512_tr0", {"DPOSER_WGRAD_TR": "0"}),              # wgrads on transposed operand copies
    # 512 samples on the 128x128 tilings: the time-branch dgrad keeps its k-split form (``wgrad_b512``)
    ("wgrad_b512", SP.POLICY_MID), ("wgrad_b512", MID_SPLITK),
    # ... and on the 256x256 tilings, which have the one-launch form only: the inputs of ``wgrad_b512`` with the bias gradient of
    # shared_time_embed summed before the store, which is the reference ``wgrad_b512_tr0`` holds
    ("wgrad_b512_tr0", SP.POLICY_BIG), ("wgrad_b512_tr0", BIG_SPLITK),
])
def test_parameter_gradients_over_clean_rows_vs_faithful_oracle(case, env, tuning_env):
    """Rows are independent in the dgrad and the library has no atomics.  Pass 1 finds the rows S that are clean in out and in x.grad (on
    the GPU and on the float32-arithmetic oracle); pass 2 repeats with the upstream gradient zeroed outside S: nothing rounded differs
    that reaches x.grad on S, so every parameter gradient must agree with the oracle's backward under the same masked gradient to fp32
    accumulation -- bound: 8 x what the float32-arithmetic oracle shows against the float64-arithmetic one for the same sum, per tensor
    and, for matrices, per aligned 32 x 32 tile; the 1-D gradients of the GroupNorm layers share the largest of their reference
    errors (``bf16_ref.param_grad_bounds`` says why: an x_hat flip that x.grad cannot show).
    Measured (GPU / reference, rel-L2): matrices 1.0e-7 ... 6.5e-7 / 1.6e-7 ... 6.6e-7, their tiles 2.5e-7 ... 4.7e-6 / 5.1e-7 ... 4.7e-6;
    shared_time_embed 7.9e-6 ... 3.2e-5 / 1.1e-5 ... 1.3e-5; layer vectors at most 6.2e-6."""
    m, (x, t, g) = _model(case)
    pl = _force(tuning_env, m, case, env)
    assert pl.time_split == (1 if Q.CASES[case].get("se_bias_stored", True) else 0), pl      # which of the two forms the reference of the case restates

    def run(gg):
        for q in m.parameters():
            q.grad = None
        xd = _dev(x).requires_grad_(True)
        out = m(xd, _dev(t) * 999)
        out.backward(_dev(gg))
        return out.detach(), xd.grad

    out1, dx1 = run(g)
    S = _rows(out1, case, "out") & _rows(dx1, case, "dx")
    S &= Q.reference_clean_rows(case, "out") & Q.reference_clean_rows(case, "dx")
    _log_measured("rows_in_S", float(S.sum()))
    print("rows in S:", int(S.sum()))
    assert S.sum() >= Q.S_MIN                                                  # measured 249 / 510 / 1087 / 249 (reference alone: 328 / 671 / 1463)
    St = torch.as_tensor(S)
    out2, dx2 = run(g * St[:, None].to(g.dtype))
    assert torch.equal(dx2[St.to(DEV)], dx1[St.to(DEV)]) and float(dx2[(~St).to(DEV)].abs().max()) == 0.0
    assert torch.equal(out2, out1)
    _, want = Q.masked_param_grads(case, S)
    rel_bound, tile_bound = Q.param_grad_bounds(case, S)
    for name, prm in m.named_parameters():
        if name.startswith("pre_dense_cond"):
            assert prm.grad is None or float(prm.grad.abs().max()) == 0.0
            continue
        got, w = prm.grad.detach().double().cpu(), want[name]
        e = float((got - w).norm() / w.norm())
        _log_measured("grad_rel_over_bound/" + name, e / rel_bound[name])
        print(f"{name}: rel {e:.2e} (bound {rel_bound[name]:.2e})" + (f", tile {Q.tile_err(got, w):.2e} (bound {tile_bound[name]:.2e})" if w.dim() == 2 else ""))
        assert e <= rel_bound[name], name
        if w.dim() == 2:
            assert Q.tile_err(got, w) <= tile_bound[name], name
