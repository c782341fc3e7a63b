"""dposer_pose_set_distances and the scores built on it against the float64 rule of tests/set_dist_ref.py.

Tolerance, derived: bound(J) = (J + 6) 2^-24 relative per distance -- per joint the squares' sum and the square root, across joints J - 1
adds and one multiply (tests/set_dist_ref.py).  knn_dist and sum are held to it; indices are compared exactly where the oracle's gaps to
both neighbouring ranks exceed 2 bound, elsewhere the returned index's oracle distance must match the oracle's rank distance within bound;
covered must lie between the oracle's counts at radii (1 - bound) and radii (1 + bound).  tests/test_set_dist_cpu.py asserts that the
fall-backs of the last two apply to at most 2 % of the entries of every case."""
import ctypes as C

import numpy as np
import pytest
import torch

import set_dist_ref as R
from gpu_common import DEV
from helpers import load

pytestmark = pytest.mark.gpu


def _plan(na, nb, J, k):
    from dposer_amd import _C
    out = (C.c_int32 * 4)()
    assert _C.lib().dposer_pose_set_distances_plan(na, nb, J, k, out) == 0
    return tuple(out)


CASES = R.gpu_cases(_plan)


def _run(a, b=None, **kw):
    """pose_set_distances on numpy inputs -> numpy outputs."""
    from dposer_amd.utils.metric import pose_set_distances
    dev = lambda x: None if x is None else torch.as_tensor(x).to(DEV)
    if "radii" in kw:
        kw["radii"] = dev(kw["radii"])
    out = pose_set_distances(dev(a), dev(b), **kw)
    return {key: v.cpu().numpy() for key, v in out.items()}


def _check(out, D, k, J, radii=None, same_set=False, what=""):
    """One call's outputs against the oracle's distance matrix D under the rules of this file's docstring."""
    e = R.bound(J)
    if k:
        rd, ri = R.knn(D, k, same_set)
        gd, gi = out["knn_dist"].astype(np.float64), out["knn_idx"].astype(np.int64)
        fin = np.isfinite(rd[:, :k])
        assert np.array_equal(np.isfinite(gd), fin) and np.array_equal(gi < 0, ~fin), what              # the +inf / -1 tail
        assert np.all(gd[~fin] == np.inf) and np.all(gi[~fin] == -1), what
        err = np.abs(gd[fin] - rd[:, :k][fin])
        print(f"{what}: knn_dist max rel err {(err / np.maximum(rd[:, :k][fin], 1e-300)).max() if err.size else 0.0:.3e} (bound {e:.3e})")
        assert np.all(err <= e * rd[:, :k][fin]), what
        prev = np.concatenate([np.full((rd.shape[0], 1), -np.inf), rd[:, :k - 1]], axis=1)
        with np.errstate(invalid="ignore"):                                                             # (inf - inf in the tails, masked by fin)
            assert np.all(np.diff(gd, axis=1)[fin[:, 1:]] >= 0), what                                   # ascending
            clear = fin & (rd[:, :k] - prev > 2 * e * rd[:, :k]) & (rd[:, 1:k + 1] - rd[:, :k] > 2 * e * rd[:, :k])
        assert np.array_equal(gi[clear], ri[:, :k][clear]), what
        rows = np.nonzero(fin & ~clear)
        if rows[0].size:
            back = D[rows[0], gi[rows]]                                                                 # the returned index's own distance
            assert np.all(np.abs(back - rd[:, :k][rows]) <= e * rd[:, :k][rows]), what
            if same_set:
                assert np.all(gi[rows] != rows[0]), what
    if radii is not None:
        r = np.asarray(radii, dtype=np.float64)
        lo, hi = R.covered(D, r * (1 - e), same_set), R.covered(D, r * (1 + e), same_set)
        assert np.all((lo <= out["covered"]) & (out["covered"] <= hi)), what
    if "sum" in out:
        want = R.total(D)
        err = abs(float(out["sum"]) - want) / want
        print(f"{what}: sum rel err {err:.3e} (bound {e:.3e})")
        assert err <= e, what


@pytest.mark.parametrize("na,nb,J,k,seed", CASES)
def test_outputs_match_the_oracle(na, nb, J, k, seed):
    a, b = R.make_sets(na, nb, J, seed)
    radii = R.case_radii(b)
    out = _run(a, b, k=k, radii=radii, want_sum=True)
    assert out["knn_dist"].shape == (na, k) and out["knn_idx"].dtype == np.int32 and out["covered"].shape == (na,)
    _check(out, R.distances(a, b), k, J, radii, what=f"case {(na, nb, J, k, seed)}")


def test_the_cases_run_both_paths_and_the_library_splits_some():
    plans = [_plan(na, nb, J, k) for na, nb, J, k, _ in CASES]
    assert {p[3] for p in plans} == {0, 1} and any(p[2] >= 2 for p in plans)
    assert {J for _, _, J, _, _ in CASES} == {1, 22, 23, 55, 128} and {k for _, _, _, k, _ in CASES} == {1, 3, 8}


@pytest.mark.parametrize("J", [22, 23])
def test_results_do_not_depend_on_the_split(J):
    """Forced splits 1, 2, 3, 7 and the library's own: knn_dist / knn_idx / covered bit for bit, sum within bound of the oracle; also
    with the references at one below, at and one above three whole tiles under three splits."""
    tile = _plan(193, 1031, J, 3)[1]
    for nb in (1031, 3 * tile - 1, 3 * tile, 3 * tile + 1):
        a, b = R.make_sets(193, nb, J, 60 + J)
        radii = R.case_radii(b)
        D = R.distances(a, b)
        outs = [_run(a, b, k=3, radii=radii, want_sum=True, splits=s) for s in (0, 1, 2, 3, 7)]
        for o in outs:
            _check(o, D, 3, J, radii, what=f"J {J} nb {nb}")
        for o in outs[1:]:
            for key in ("knn_dist", "knn_idx", "covered"):
                assert np.array_equal(o[key], outs[0][key]), (J, nb, key)


@pytest.mark.parametrize("J", [22, 23])
def test_same_set_is_the_general_path_without_the_own_column(J):
    """b = None against b = a.clone() with the own column taken out by hand: k + 1 neighbours asked for, the own index dropped (or
    the last entry where it is not among them), covered less the own column (distance 0 <= any radius); and the oracle's same-set
    rule, including k > nb - 1 for the +inf / -1 tail."""
    n, k = 600, 3
    a, _ = R.make_sets(n, 1, J, 70 + J)
    radii = R.case_radii(a)
    same = _run(a, None, k=k, radii=radii, want_sum=True)
    full = _run(a, a.copy(), k=k + 1, radii=radii, want_sum=True)
    own = full["knn_idx"] == np.arange(n)[:, None]
    own[~own.any(1), k] = True
    keep = ~own
    assert np.array_equal(full["knn_idx"][keep].reshape(n, k), same["knn_idx"])
    assert np.array_equal(full["knn_dist"][keep].reshape(n, k), same["knn_dist"])
    assert np.array_equal(full["covered"] - 1, same["covered"])
    assert same["sum"] == full["sum"]                                  # both full forms (neighbours were asked for): the same order
    D = R.distances(a, a)
    _check(same, D, k, J, radii, same_set=True, what=f"same set J {J}")
    # APD: the symmetric form (sum alone) against the full form and the oracle
    sym = _run(a, None, want_sum=True)
    e = R.bound(J)
    assert abs(float(sym["sum"]) - float(same["sum"])) <= e * float(same["sum"])
    assert abs(float(sym["sum"]) - R.total(D)) <= e * R.total(D)
    small = a[:5]
    out = _run(small, None, k=8, radii=radii[:5])
    _check(out, R.distances(small, small), 8, J, radii[:5], same_set=True, what="k > n - 1")
    assert np.all(out["knn_idx"][:, 4:] == -1) and np.all(np.isinf(out["knn_dist"][:, 4:])) and np.all(out["knn_idx"][:, :4] >= 0)


@pytest.mark.parametrize("J", [22, 23])
def test_equal_distances_go_to_the_smaller_index(J):
    """References 65 .. 129 repeat references 0 .. 64: every distance appears twice, bit for bit, in different tiles and (under
    forced splits) in different splits.  And in the same set a copy of a_i elsewhere is its neighbour at distance 0."""
    a, b0 = R.make_sets(70, 65, J, 80 + J)
    b = np.concatenate([b0, b0])
    for splits in (1, 2, 3):
        out = _run(a, b, k=8, splits=splits)
        d, i = out["knn_dist"], out["knn_idx"]
        assert np.array_equal(d[:, 0::2], d[:, 1::2]) and np.array_equal(i[:, 0::2] + 65, i[:, 1::2]), (J, splits)
    s = a.copy()
    s[41] = s[3]
    out = _run(s, None, k=2)
    assert out["knn_idx"][3, 0] == 41 and out["knn_idx"][41, 0] == 3 and out["knn_dist"][3, 0] == 0.0 and out["knn_dist"][41, 0] == 0.0
    assert np.all(out["knn_idx"] != np.arange(70)[:, None])


@pytest.mark.parametrize("J", [22, 23])
def test_a_nan_reference_is_never_returned_and_never_covers(J):
    a, b = R.make_sets(70, 100, J, 90 + J)
    b[10] = np.nan
    b[77, 3, 1] = np.nan
    radii = np.full((100,), np.inf, dtype=np.float32)
    out = _run(a, b, k=8, radii=radii, want_sum=True)
    assert not np.isin(out["knn_idx"], [10, 77]).any() and np.isfinite(out["knn_dist"]).all()
    assert np.all(out["covered"] == 98) and np.isnan(out["sum"])
    fin = np.delete(np.arange(100), [10, 77])
    clean = _run(a, b[fin], k=8)
    assert np.array_equal(out["knn_dist"], clean["knn_dist"]) and np.array_equal(fin[clean["knn_idx"]], out["knn_idx"])


def test_two_calls_return_the_same_bits():
    a, b = R.make_sets(300, 1100, 22, 5)
    radii = R.case_radii(b)
    first, second = (_run(a, b, k=3, radii=radii, want_sum=True) for _ in range(2))
    for key in ("knn_dist", "knn_idx", "covered", "sum"):
        assert np.array_equal(first[key], second[key]), key
    s1, s2 = (_run(a, None, want_sum=True)["sum"] for _ in range(2))
    assert s1 == s2


def test_more_than_2_32_pairs():
    """J = 1, a_i = (i, 0, 0), b_j = (j + 0.25, 0, 0), n = 2^16 + 1 of each: n^2 > 2^32 pairs, every value exact in fp32.  The nearest
    reference of a_i is b_i at 0.25, the second b_(i-1) at 0.75 (b_1 at 1.25 for i = 0); radius 0.5 covers exactly one; the sum from
    cumulative sums: row i holds m - 0.25 for m = 1 .. i and m + 0.25 for m = 0 .. n - 1 - i."""
    n = (1 << 16) + 1
    i = np.arange(n, dtype=np.float64)
    a = np.zeros((n, 1, 3), dtype=np.float32)
    b = np.zeros((n, 1, 3), dtype=np.float32)
    a[:, 0, 0] = i
    b[:, 0, 0] = i + 0.25
    out = _run(a, b, k=2, radii=np.full((n,), 0.5, dtype=np.float32), want_sum=True)
    idx = np.arange(n)
    assert np.array_equal(out["knn_idx"][:, 0], idx) and np.all(out["knn_dist"][:, 0] == 0.25)
    assert np.array_equal(out["knn_idx"][1:, 1], idx[:-1]) and np.all(out["knn_dist"][1:, 1] == 0.75)
    assert out["knn_idx"][0, 1] == 1 and out["knn_dist"][0, 1] == 1.25
    assert np.all(out["covered"] == 1)
    tri = np.concatenate([[0.0], np.cumsum(i[1:])])                   # tri[m] = 1 + 2 + ... + m
    below = tri - 0.25 * i                                            # sum over m = 1 .. i of (m - 0.25)
    above = tri[::-1] + 0.25 * (n - i)                                # sum over m = 0 .. n - 1 - i of (m + 0.25)
    want = float((below + above).sum())
    assert abs(float(out["sum"]) - want) <= R.bound(1) * want


def test_apd_wrapper_against_the_torch_apd():
    """Both are fp32 evaluations of the same mean, each within bound(J) of the exact value plus its own final rounding."""
    from dposer_amd.utils.metric import average_pairwise_distance, average_pairwise_distance_hip
    g = load("g12_likelihood_ode")
    tol = 2 * R.bound(22) + 2.0 ** -23
    for joints in (g["apd/joints"], R.make_sets(500, 1, 22, 3)[0]):
        j = torch.tensor(joints, device=DEV)
        got, ref = average_pairwise_distance_hip(j), average_pairwise_distance(j)
        assert got.shape == () and got.dtype == torch.float32 and got.is_cuda
        exact = R.total(R.distances(joints, joints)) / (len(joints) * (len(joints) - 1))
        assert abs(float(got) - float(ref)) <= tol * exact
        assert abs(float(got) - exact) <= (R.bound(22) + 2.0 ** -24) * exact
    assert abs(float(average_pairwise_distance_hip(torch.tensor(g["apd/joints"], device=DEV))) - float(g["apd/value"])) < 1e-6


def test_nearest_pose_distance_wrapper():
    from dposer_amd.utils.metric import nearest_pose_distance
    q, ref = R.make_sets(130, 400, 22, 4)
    d, i = nearest_pose_distance(torch.tensor(q, device=DEV), torch.tensor(ref, device=DEV), k=3)
    assert d.shape == (130, 3) and i.shape == (130, 3) and d.is_cuda and i.dtype == torch.int32
    _check({"knn_dist": d.cpu().numpy(), "knn_idx": i.cpu().numpy()}, R.distances(q, ref), 3, 22, what="nearest_pose_distance")


def test_generation_fidelity_against_the_oracle():
    """(N, M, k) = (257, 193, 3).  The wrapper's radii are themselves device distances, so a comparison d <= r carries the error of both
    sides: the counts lie between the oracle's at radii (1 - s) and radii (1 + s) with s = 2 bound + bound^2 < 2.01 bound."""
    from dposer_amd.utils.metric import generation_fidelity
    J, k = 22, 3
    G, Rl = R.make_sets(257, 193, J, 8)
    got = {key: float(v) for key, v in generation_fidelity(torch.tensor(G, device=DEV), torch.tensor(Rl, device=DEV), k=k).items()}
    e = R.bound(J)
    lo, mid, hi = R.fidelity(G, Rl, k, -2.01 * e), R.fidelity(G, Rl, k), R.fidelity(G, Rl, k, 2.01 * e)
    print("generation_fidelity:", got, "oracle:", mid)
    assert set(got) == {"APD", "dNN", "precision", "recall", "density", "coverage"}
    for key in ("APD", "dNN"):
        assert abs(got[key] - mid[key]) <= (e + 2.0 ** -24) * mid[key], key
    for key in ("precision", "recall", "density", "coverage"):
        assert lo[key] * (1 - 2.0 ** -23) <= got[key] <= hi[key] * (1 + 2.0 ** -23), (key, lo[key], got[key], hi[key])
    assert 0 < mid["precision"] and 0 < mid["recall"] and 0 < mid["coverage"] < 1          # (the case is not a trivial one)


def test_validate_with_fidelity_keeps_the_old_keys_and_adds_the_new():
    """tasks.train.validate on the tiny configuration of tests/test_gpu_train_loop.py: fidelity_k = 3 adds finite scores computed from
    all generated samples; the keys and values of a run with fidelity_k = 0 under the same seeds are unchanged."""
    from test_gpu_train_loop import ToySet, _body, _config
    from dposer_amd.algorithms.advanced import losses
    from dposer_amd.algorithms.ema import ExponentialMovingAverage
    from dposer_amd.tasks.train import build_model, build_sde, validate
    cfg = _config()
    test_set = ToySet(50, 50)
    body = _body()
    torch.manual_seed(7)
    model = build_model(cfg).to(DEV)
    state = dict(optimizer=losses.get_optimizer(cfg, model.parameters()), model=model,
                 ema=ExponentialMovingAverage(model.parameters(), decay=cfg.model.ema_rate), step=0)
    sde = build_sde(cfg)[0]
    runs = []
    for fk in (0, 3):
        torch.manual_seed(11)
        runs.append(validate(state, sde, cfg, test_set.poses, body, test_set.Denormalize, device=DEV, fidelity_k=fk))
    old, new = runs
    assert set(old) == {"bpd", "mpvpe_all", "mpjpe_body", "APD"}
    assert set(new) == set(old) | {"APD_all", "dNN", "precision", "recall", "density", "coverage"}
    assert all(new[key] == old[key] for key in old)
    print("validate(fidelity_k=3):", new)
    assert all(isinstance(v, float) and np.isfinite(v) for v in new.values())
