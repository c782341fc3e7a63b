"""The rounding-faithful bf16 oracle (tests/bf16_ref.py) is right before any GPU sees it: without rounding it IS the plain oracle, its
designed error is the one the project measured, every rounding point it models moves it, and on the reference alone
(float32 arithmetic against float64 arithmetic) each case of tests/test_gpu_bf16_faithful.py splits into clean and flipped rows."""
import numpy as np
import pytest
import torch

import bf16_ref as Q
from oracle import score_ref as R
from weights import make_weights

torch.set_num_threads(8)


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@pytest.mark.parametrize("masks", [False, True])
@pytest.mark.parametrize("nb,D", [(1, 63), (2, 63), (1, 126), (2, 126)])
def test_without_rounding_the_oracle_is_the_plain_oracle_and_its_backward_is_autograd(nb, D, masks):
    B, drop_p = 40, 0.3
    p = Q.case_weights(3, D, nb)
    x, t, g = Q.case_inputs(0, B, D)
    keep = [torch.tensor((np.random.RandomState(5 + i).rand(B, Q.H) < 1 - drop_p).astype(np.float32)) for i in range(1 + 2 * nb)] if masks else None
    names = R.param_names(n_blocks=nb)
    p64 = {k: v.double() for k, v in p.items()}
    leaves = {n: p64[n].clone().requires_grad_(True) for n in names}
    xr = x.double().requires_grad_(True)
    ref = R.scorefc_forward({**p64, **leaves}, xr, (t * 999).double(), n_blocks=nb, drop_masks=keep, drop_p=drop_p if masks else 0.0)
    want = torch.autograd.grad((ref * g.double()).sum(), [xr] + [leaves[n] for n in names], allow_unused=True)
    tape = {}
    out = Q.forward(p, x, t * 999, n_blocks=nb, keep=keep, drop_p=drop_p if masks else 0.0, rounding=None, tape=tape)
    dx, grads = Q.backward(tape, g)
    ref = ref.detach()
    assert float((out - ref).abs().max() / ref.abs().max()) <= 1e-12            # float64 round-off of another operation order: measured 7e-16
    assert _rel(dx, want[0]) <= 1e-10                                            # measured 1e-15
    assert set(grads) == set(names)
    for n, w in zip(names, want[1:]):
        if w is None:
            assert n.startswith("pre_dense_cond") and float(grads[n].abs().max()) == 0.0
        else:
            assert grads[n].shape == w.shape and _rel(grads[n], w) <= 1e-10, n   # measured 1.1e-15


def test_designed_error_is_the_error_the_project_measured():
    """Shipped shape, seed-1 weights, the inputs of the parity measurement (bf16 forward 4.8e-3 against the fp32
    goldens): the faithful oracle must lie that far from the plain one, i.e. the modelled roundings are the mode's error."""
    w = make_weights(1, D=63)
    w["sigmas"] = R.sigma_table()
    rs = np.random.RandomState(0)
    x = torch.tensor(rs.standard_normal((200, 63)).astype(np.float32))
    t = torch.tensor(rs.uniform(1e-3, 1, 200).astype(np.float32))
    d = _rel(Q.forward(w, x, t * 999, n_blocks=2), Q.forward(w, x, t * 999, n_blocks=2, rounding=None))
    print(f"designed error {d:.3e}")
    assert 0.7 * 4.8e-3 <= d <= 1.4 * 4.8e-3                                     # measured 4.57e-3


def test_every_modelled_rounding_moves_the_oracle():
    """Truncation instead of round-to-nearest, and leaving out any single rounding point, moves what depends on that point by more than
    10 tau (tau = 8 e_ref of the record: the clean-row threshold of the GPU tests) -- so a kernel that rounds differently at one
    point cannot have clean rows.  Forward points move out; the points of the dgrad chain move dx; u and dU (time-branch dgrad) move
    the gradient of shared_time_embed."""
    nb, B = 1, 64
    p = Q.case_weights(8, 63, nb)
    x, t, g = Q.case_inputs(0, B, 63)

    def run(**kw):
        tape = {}
        out = Q.forward(p, x, t * 999, n_blocks=nb, tape=tape, **kw)
        dx, gr = Q.backward(tape, g)
        return dict(out=out, dx=dx, se=gr["shared_time_embed.0.weight"])

    tau = Q.TAU_FACTOR * max(r["e_ref"] for rec in Q.RECORD.values() for r in rec.values() if isinstance(r, dict))
    base = run()
    moved = {k: _rel(v, base[k]) for k, v in run(rounding="trunc").items()}
    print("trunc", moved)
    assert min(moved.values()) > 10 * tau                                        # measured 1.1e-2 (the bound of today's tests)
    for name in Q.point_names(nb):
        what = "se" if name in ("upre", "dU") else ("dx" if name in Q.BACKWARD_POINTS else "out")
        d = _rel(run(skip=name)[what], base[what])
        print(name, what, f"{d:.2e}")
        assert d > 10 * tau, name                                                # measured 1.5e-3 ... 5.8e-3; 10 tau = 2.1e-5


def test_one_wrong_dropout_decision_moves_its_row():
    """One keep decision of one dropout site inverted in every row (what a lost bit of the GnAux record or of the AND mask would do):
    the rows of the train-form output move by 10 tau and more in the median and too few stay within tau for rule (b)."""
    case = "drop05_b200"
    c = Q.CASES[case]
    p = Q.case_weights(c["wseed"], c["D"], c["nb"])
    x, t, _ = Q.case_inputs(c["seed"], c["B"], c["D"])
    keep = Q.dropout_masks(case)
    base = Q.reference(case)["out"]
    tau = Q.TAU_FACTOR * Q.RECORD[case]["out"]["e_ref"]
    for site in range(len(keep)):
        wrong = [k.clone() for k in keep]
        wrong[site][:, 37] = 1 - wrong[site][:, 37]
        moved = Q.row_err(Q.forward(p, x, t * 999, n_blocks=c["nb"], keep=wrong, drop_p=c["drop_p"]), base)
        print(site, f"min {moved.min():.2e} median {np.median(moved):.2e} share above tau {(moved > tau).mean():.3f}")
        assert np.median(moved) > 10 * tau                                       # measured 7.7e-3 ... 1.0e-2 (10 tau = 1.4e-5)
        # (an inverted decision on a SiLU value near zero moves little: the smallest row 1.2e-5) -- rule (b) needs a clean share of
        # p_ref^3 = 0.74; at most this many rows stay within tau: measured none
        assert (moved <= tau).mean() < Q.RECORD[case]["out"]["p_ref"] ** 3


@pytest.mark.parametrize("case", list(Q.CASES))
def test_the_row_split_exists_on_the_reference_alone(case):
    """float32 arithmetic against float64 arithmetic of the same oracle, for every GPU case: the conditions of
    ``bf16_ref.unmet_conditions`` hold, and the committed RECORD (which the GPU tests read) is what ``regenerate`` gives -- up to what
    another BLAS summation order moves in the float32 run."""
    rec = Q.regenerate(case)
    print(Q.format_record({case: rec}))
    assert Q.unmet_conditions(case, rec) == []
    assert Q.unmet_conditions(case, Q.RECORD[case]) == []
    for n in Q.compared(case):
        got, com = rec[n], Q.RECORD[case][n]
        assert com["d_max"] == pytest.approx(got["d_max"], rel=1e-3)            # float64 on both sides
        assert com["e_ref"] / 1.5 <= got["e_ref"] <= com["e_ref"] * 1.5         # a maximum over rows of fp32 summation error
        assert com["el_ref"] / 1.5 <= got["el_ref"] <= com["el_ref"] * 1.5
        assert abs(com["p_ref"] - got["p_ref"]) <= 0.03 and abs(com["flip_free"] - got["flip_free"]) <= 0.03
    if Q.CASES[case]["kind"] == "wgrad":
        assert abs(rec["S"] - Q.RECORD[case]["S"]) <= 0.03 * Q.CASES[case]["B"]
