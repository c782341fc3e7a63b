"""The float64 statement of the pose-set distance rules of include/dposer_hip.h (dposer_pose_set_distances) and of the scores
utils.metric builds on them, the generator of the test inputs and the list of cases the GPU test runs.  Test infrastructure: the
package never imports it."""
import numpy as np


def bound(J):
    """Relative error allowed on one fp32 distance of J joints: per joint the squares' sum and the square root, across joints J - 1
    adds and one multiply -- (J + 6) half-ulps."""
    return (J + 6) * 2.0 ** -24


def make_sets(na, nb, J, seed):
    """Two fp32 pose sets around one skeleton: base = 0.3 N(0,1) [J,3]; pose = base * U(0.5, 1.5) + 0.05 N(0,1).  The per-sample scale
    spreads the distances (iid Gaussian joints concentrate them at large J, and near-ties grow)."""
    rs = np.random.RandomState(seed)
    base = 0.3 * rs.standard_normal((J, 3))

    def draw(n):
        return (base[None] * rs.uniform(0.5, 1.5, (n, 1, 1)) + 0.05 * rs.standard_normal((n, J, 3))).astype(np.float32)

    return draw(na), draw(nb)


def distances(a, b, chunk=64):
    """[na, nb] float64: d(a_i, b_j) = mean over joints of ||a_i - b_j||."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    out = np.empty((a.shape[0], b.shape[0]))
    for lo in range(0, a.shape[0], chunk):
        out[lo:lo + chunk] = np.sqrt(((a[lo:lo + chunk, None] - b[None]) ** 2).sum(-1)).mean(-1)
    return out


def _candidates(D, same_set):
    """D with what can never be a neighbour (the own index of a same-set row, NaN) set to +inf."""
    C = np.where(np.isnan(D), np.inf, D)
    if same_set:
        C = C.copy()
        np.fill_diagonal(C, np.inf)
    return C


def knn(D, k, same_set=False):
    """(dist [na, k], idx [na, k]): the k smallest distances of each row, ascending, ties to the smaller index; fewer than k
    candidates: tail +inf / -1.  With more than k columns one extra rank is appended (column k) so that callers can read the gap
    behind rank k."""
    C = _candidates(D, same_set)
    order = np.argsort(C, axis=1, kind="stable")[:, :k + 1]
    d = np.take_along_axis(C, order, axis=1)
    idx = np.where(np.isinf(d), -1, order).astype(np.int64)
    pad = k + 1 - d.shape[1]
    if pad > 0:
        d = np.concatenate([d, np.full((d.shape[0], pad), np.inf)], axis=1)
        idx = np.concatenate([idx, np.full((idx.shape[0], pad), -1, dtype=np.int64)], axis=1)
    return d, idx


def covered(D, radii, same_set=False):
    """[na] counts of j with d(a_i, b_j) <= radii[j] (a NaN never covers; same set: j = i left out)."""
    with np.errstate(invalid="ignore"):
        hit = D <= np.asarray(radii, dtype=np.float64)[None]                # (False for a NaN distance, whatever the radius)
    if same_set:
        hit = hit & ~np.eye(D.shape[0], D.shape[1], dtype=bool)
    return hit.sum(1)


def total(D):
    return float(D.sum())


def kth_radius(X, k):
    """Distance of every pose of X to its k-th nearest neighbour inside X, itself excluded."""
    return knn(distances(X, X), k, same_set=True)[0][:, k - 1]


def fidelity(G, R, k, slack=0.0):
    """The scores of utils.metric.generation_fidelity in float64.  ``slack`` scales every radius by (1 + slack): a negative and a
    positive slack bracket what a computation with that relative error on distances and radii may return."""
    N = G.shape[0]
    DGR = distances(G, R)
    rR, rG = kth_radius(R, k) * (1 + slack), kth_radius(G, k) * (1 + slack)
    cov_g = (DGR <= rR[None]).sum(1)
    DGG = distances(G, G)
    return {"APD": DGG.sum() / (N * (N - 1)), "dNN": DGR.min(1).mean(), "precision": (cov_g > 0).mean(),
            "recall": ((DGR.T <= rG[None]).sum(1) > 0).mean(), "density": cov_g.sum() / (k * N),
            "coverage": (DGR.min(0) <= rR).mean()}


def case_radii(b, k=3):
    """The radii a case's covered output is asked with: each reference's distance to its min(k, nb - 1)-th neighbour inside B, as the
    fp32 values the device reads (0.3 for a single reference)."""
    nb = b.shape[0]
    if nb == 1:
        return np.full((1,), 0.3, dtype=np.float32)
    return kth_radius(b, min(k, nb - 1)).astype(np.float32)


def near_tie_share(D, k, J, factor=2.0, same_set=False):
    """Share of (row, rank <= k) whose relative gap to the next rank is below factor * bound(J)."""
    d, _ = knn(D, k, same_set)
    head, nxt = d[:, :k], d[:, 1:k + 1]
    ok = np.isfinite(head) & np.isfinite(nxt)
    gap = np.where(ok, nxt - np.where(ok, head, 0.0), np.inf)
    return float((gap < factor * bound(J) * np.where(ok, head, 1.0)).mean())


def covered_flip_share(D, radii, J, factor=1.0, same_set=False):
    """Share of rows whose covered count differs between radii * (1 - factor * bound) and radii * (1 + factor * bound)."""
    r = np.asarray(radii, dtype=np.float64)
    e = factor * bound(J)
    return float((covered(D, r * (1 - e), same_set) != covered(D, r * (1 + e), same_set)).mean())


def gpu_cases(plan):
    """(na, nb, J, k, seed) of every case of tests/test_gpu_set_dist.py::test_outputs_match_the_oracle.  ``plan(na, nb, J, k)`` returns
    dposer_pose_set_distances_plan's four numbers: the sizes sit one below, at and one above the rows of a workgroup and the references
    of a tile of either path, and around a whole number of tiles (where the library's own splits end); na = 1 and nb = 1 close the list."""
    rows, t_reg, _, reg = plan(1000, 1000, 22, 1)
    _, t_gen, _, gen = plan(1000, 1000, 23, 1)
    assert reg == 1 and gen == 0
    cases = [(193, 1031, 22, 3, 1), (65, 257, 1, 1, 2), (129, 513, 55, 8, 3), (67, 300, 128, 3, 4), (257, 257, 23, 3, 5),
             (1, 1025, 22, 8, 6), (300, 9, 22, 3, 7)]
    for d, k in ((-1, 1), (0, 3), (1, 8)):
        cases.append((rows + d, t_reg + d, 22, k, 10 + d))
        cases.append((rows + d, t_gen + d, (23, 1, 55)[d + 1], k, 20 + d))
        cases.append((33, 8 * t_reg + d, 22, k, 30 + d))                       # eight whole tiles, one reference either way
        cases.append((33, 8 * t_gen + d, (55, 23, 1)[d + 1], k, 40 + d))
    cases.append((40, 1, 22, 1, 50))
    cases.append((40, 1, 23, 3, 51))
    return cases
