"""Test infrastructure: the mesh self-intersection rule of dposer_mesh_self_intersections (include/dposer_hip.h) in numpy fp64, with a KD-tree
broad phase, and a three-way verdict per face.

Every pair predicate is evaluated together with a margin: how far (as a length, relative to the mesh's bounding-box diagonal L) its value is
from a sign change.  A pair whose result rests on a value within TOL * L of a sign change (exact zeros excepted: they come from exactly
representable configurations, which fp32 computes exactly too) is ambiguous.  Per face:
    flagged   -- some pair surely intersects;
    clean     -- every pair surely does not;
    ambiguous -- neither: the face is decided only through ambiguous pairs.
The GPU's fp32 flags must equal the oracle on every face that is not ambiguous."""
import numpy as np
from scipy.spatial import cKDTree

TOL = 1e-6
BARY_EPS = 1e-6


def _cross(a, b):
    return np.cross(a, b)


def _dot(a, b):
    return np.einsum("...i,...i->...", a, b)


def _norm(a):
    return np.sqrt(_dot(a, a))


class _Verdict:
    """Per-pair (sure_true, sure_false) accumulated through conjunctions of margin-carrying conditions."""

    @staticmethod
    def conj(margins, tol):
        """AND of conditions with signed margins (> 0: holds); +inf / -inf: exact.  Returns (sure_true, sure_false)."""
        m = np.stack(margins, axis=0)
        return (m > tol).all(axis=0), (m < -tol).any(axis=0)


def _seg_interior(A, B, q0, q1, q2, tol):
    """Segment A -> B crosses triangle (q0, q1, q2) strictly inside: (sure_true, sure_false)."""
    e1, e2, d = q1 - q0, q2 - q0, B - A
    pv = _cross(d, e2)
    det = _dot(e1, pv)
    n = _cross(e1, e2)
    nn = _norm(n)
    dl = _norm(d)
    par = det == 0
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.where(par, 0.0, 1.0 / np.where(par, 1.0, det))
        tv = A - q0
        b1 = _dot(tv, pv) * inv
        qv = _cross(tv, e1)
        b2 = _dot(d, qv) * inv
        t = _dot(e2, qv) * inv
        h1, h2, h0 = nn / _norm(e2), nn / _norm(e1), nn / _norm(q2 - q1)
    inf = np.inf

    def exact(m, v, inclusive_at):
        return np.where(v == inclusive_at, inf, m)
    margins = [np.where(par, -inf, inf),
               exact(t * dl, t, 0.0), exact((1 - t) * dl, t, 1.0),
               (b1 - BARY_EPS) * h1, (b2 - BARY_EPS) * h2, (1 - b1 - b2) * h0]
    margins = [np.where(par, -inf, m) for m in margins]
    st, sf = _Verdict.conj(margins, tol)
    return st, sf


def _shared_vertex(P, k, Q, tol):
    """Face P (corners [n, 3, 3]) sharing its corner k [n] with face Q."""
    idx = np.arange(len(P))
    s, a, b = P[idx, k], P[idx, (k + 1) % 3], P[idx, (k + 2) % 3]
    A, B = 0.5 * s + 0.5 * a, 0.5 * s + 0.5 * b
    return _seg_interior(A, B, Q[:, 0], Q[:, 1], Q[:, 2], tol)


def _interval(p, d):
    """Moller's COMPUTE_INTERVALS (p, d [n, 3]); returns lo, hi, coplanar mask."""
    ss = lambda a, b: ((a > 0) & (b > 0)) | ((a < 0) & (b < 0))
    k = np.full(len(p), -1)
    c = [ss(d[:, 0], d[:, 1]), ss(d[:, 0], d[:, 2]), ss(d[:, 1], d[:, 2]) | (d[:, 0] != 0), d[:, 1] != 0, d[:, 2] != 0]
    for cond, kk in zip(c, (2, 1, 0, 1, 2)):
        k = np.where((k < 0) & cond, kk, k)
    cop = k < 0
    k = np.where(cop, 0, k)
    k1, k2 = np.where(k == 0, 1, 0), np.where(k == 2, 1, 2)
    i = np.arange(len(p))
    pk, dk = p[i, k], d[i, k]
    with np.errstate(divide="ignore", invalid="ignore"):
        t0 = pk + (p[i, k1] - pk) * dk / (dk - d[i, k1])
        t1 = pk + (p[i, k2] - pk) * dk / (dk - d[i, k2])
    return np.minimum(t0, t1), np.maximum(t0, t1), cop


def _coplanar(n, V, U, L, tol):
    """Moller's coplanar test, vectorised; (result, min margin over its 2-D predicates / L; exact zeros excepted)."""
    a = np.abs(n)
    i0 = np.where(a[:, 0] > a[:, 1], np.where(a[:, 0] > a[:, 2], 1, 0), 0)
    i1 = np.where(a[:, 0] > a[:, 1], np.where(a[:, 0] > a[:, 2], 2, 1), np.where(a[:, 2] > a[:, 1], 1, 2))
    r = np.arange(len(n))
    X = lambda P: P[r, i0]
    Y = lambda P: P[r, i1]
    res = np.zeros(len(n), bool)
    mins = np.full(len(n), np.inf)

    def m(v):
        nonlocal mins
        mins = np.minimum(mins, np.where(v == 0, np.inf, np.abs(v) / L))

    for (va, vb) in ((0, 1), (1, 2), (2, 0)):
        Ax, Ay = X(V[:, vb]) - X(V[:, va]), Y(V[:, vb]) - Y(V[:, va])
        for (ua, ub) in ((0, 1), (1, 2), (2, 0)):
            Bx, By = X(U[:, ua]) - X(U[:, ub]), Y(U[:, ua]) - Y(U[:, ub])
            Cx, Cy = X(V[:, va]) - X(U[:, ua]), Y(V[:, va]) - Y(U[:, ua])
            f, d = Ay * Bx - Ax * By, By * Cx - Bx * Cy
            e = Ax * Cy - Ay * Cx
            for v in (f, d, d - f, e, e - f):
                m(v)
            ok = ((f > 0) & (d >= 0) & (d <= f)) | ((f < 0) & (d <= 0) & (d >= f))
            ok &= np.where(f > 0, (e >= 0) & (e <= f), (e <= 0) & (e >= f))
            res |= ok

    def pit(p, T):
        ds = []
        for (ea, eb) in ((0, 1), (1, 2), (2, 0)):
            aa = Y(T[:, eb]) - Y(T[:, ea])
            bb = -(X(T[:, eb]) - X(T[:, ea]))
            cc = -aa * X(T[:, ea]) - bb * Y(T[:, ea])
            ds.append(aa * X(p) + bb * Y(p) + cc)
        for v in ds:
            m(v)
        ss = lambda x, y: ((x > 0) & (y > 0)) | ((x < 0) & (y < 0))
        return ss(ds[0], ds[1]) & ss(ds[0], ds[2])

    res |= pit(V[:, 0], U) | pit(U[:, 0], V)
    return res, mins


def _tri_tri(V, U, L, tol):
    """Moller's test on pairs (V, U [n, 3, 3]): (sure_true, sure_false).

    A plane distance within tol of zero (and not exactly zero) is clamped to zero: the interval ends move continuously with it, so the
    clamped intervals decide the pair unless the clamping could also flip the all-on-one-side rejection or the coplanar branch."""
    n1 = _cross(V[:, 1] - V[:, 0], V[:, 2] - V[:, 0])
    du = _dot(n1[:, None], U - V[:, :1])
    n2 = _cross(U[:, 1] - U[:, 0], U[:, 2] - U[:, 0])
    dv = _dot(n2[:, None], V - U[:, :1])
    with np.errstate(divide="ignore", invalid="ignore"):
        mu = np.where(du == 0, np.inf, np.abs(du) / _norm(n1)[:, None])
        mv = np.where(dv == 0, np.inf, np.abs(dv) / _norm(n2)[:, None])
    nu, nv = mu <= tol, mv <= tol                           # near zero, not exactly zero
    cu, cv = np.where(nu, 0.0, du), np.where(nv, 0.0, dv)
    allsame = lambda d: ((d > 0).all(1)) | ((d < 0).all(1))
    sure_rej = (allsame(du) & ~nu.any(1)) | (allsame(dv) & ~nv.any(1))
    # a perturbation of the near-zero distances could reject: the others all on one side, no exact zero
    one_side = lambda c, d: (((c >= 0).all(1)) | ((c <= 0).all(1))) & (d != 0).all(1)
    poss_rej = (nu.any(1) & one_side(cu, du)) | (nv.any(1) & one_side(cv, dv))
    D = _cross(n1, n2)
    ad = np.abs(D)
    ax = np.where(ad[:, 1] > ad[:, 0], np.where(ad[:, 2] > ad[:, 1], 2, 1), np.where(ad[:, 2] > ad[:, 0], 2, 0))
    r = np.arange(len(V))
    a0, a1, cop_v = _interval(V[r, :, ax], cv)
    b0, b1, cop_u = _interval(U[r, :, ax], cu)
    cop = cop_v | cop_u
    near = nu.any(1) | nv.any(1)
    gap = np.maximum(b0 - a1, a0 - b1)                      # > 0: separated
    mg = np.where((gap == 0) & ~near, np.inf, np.abs(gap))
    res = ~(gap > 0)
    sure_true = ~sure_rej & ~poss_rej & ~cop & res & (mg > tol)
    sure_false = sure_rej | (~cop & ~res & (mg > tol))
    exact_cop = cop & ~near                                 # coplanar in exact arithmetic (every distance exactly zero)
    if exact_cop.any():
        cres, cm = _coplanar(n1[exact_cop], V[exact_cop], U[exact_cop], L, tol)
        sure_true[exact_cop] = cres & (cm > tol)
        sure_false[exact_cop] = ~cres & (cm > tol)
    return sure_true, sure_false


def candidate_pairs(P, valid, pad):
    """Pairs (i < j) of valid faces whose corners could meet within `pad`: centroid distance <= r_i + r_j + pad."""
    c = P.mean(axis=1)
    rad = np.sqrt(((P - c[:, None]) ** 2).sum(-1)).max(1)
    idx = np.nonzero(valid)[0]
    if len(idx) < 2:
        return np.zeros((0, 2), np.int64)
    tree = cKDTree(c[idx])
    pr = tree.query_pairs(2 * rad[idx].max() + pad, output_type="ndarray")
    i, j = idx[pr[:, 0]], idx[pr[:, 1]]
    keep = np.sqrt(((c[i] - c[j]) ** 2).sum(-1)) <= rad[i] + rad[j] + pad
    return np.stack([i[keep], j[keep]], 1)


def classify(vertices, faces, tol_rel=TOL):
    """vertices [V, 3] (float32 values), faces [F, 3] int: (flagged, clean, ambiguous) bool [F] and the candidate count."""
    Vx = np.asarray(vertices, dtype=np.float32).astype(np.float64)
    Fi = np.asarray(faces, dtype=np.int64)
    F = len(Fi)
    P = Vx[Fi]                                              # [F, 3, 3]
    valid = (Fi[:, 0] != Fi[:, 1]) & (Fi[:, 1] != Fi[:, 2]) & (Fi[:, 0] != Fi[:, 2])
    L = float(np.linalg.norm(Vx.max(0) - Vx.min(0))) or 1.0
    tol = tol_rel * L
    pr = candidate_pairs(P, valid, 4 * tol)
    i, j = pr[:, 0], pr[:, 1]
    lo, hi = P.min(1), P.max(1)
    meet = ((lo[i] <= hi[j]) & (lo[j] <= hi[i])).all(1)     # closed boxes: the GPU's exact rejection
    i, j = i[meet], j[meet]
    fi, fj = Fi[i], Fi[j]
    eq = fi[:, :, None] == fj[:, None, :]                   # [n, 3, 3]
    shared = eq.sum((1, 2))
    sure_t = np.zeros(len(i), bool)
    sure_f = np.zeros(len(i), bool)
    sure_t[shared == 3] = True
    sure_f[shared == 2] = True
    s1 = np.nonzero(shared == 1)[0]
    if len(s1):
        kf = eq[s1].any(2).argmax(1)
        kg = eq[s1].any(1).argmax(1)
        t1, f1 = _shared_vertex(P[i[s1]], kf, P[j[s1]], tol)
        t2, f2 = _shared_vertex(P[j[s1]], kg, P[i[s1]], tol)
        sure_t[s1] = t1 | t2
        sure_f[s1] = f1 & f2
    s0 = np.nonzero(shared == 0)[0]
    if len(s0):
        ki, kj = np.sort(fi[s0], 1), np.sort(fj[s0], 1)
        less = np.zeros(len(s0), bool)
        decided = np.zeros(len(s0), bool)
        for c in range(3):
            lt, gt = ki[:, c] < kj[:, c], ki[:, c] > kj[:, c]
            less |= ~decided & lt
            decided |= lt | gt
        A = np.where(less[:, None, None], P[i[s0]], P[j[s0]])
        B = np.where(less[:, None, None], P[j[s0]], P[i[s0]])
        t0, f0 = _tri_tri(A, B, L, tol)
        sure_t[s0], sure_f[s0] = t0, f0
    flagged = np.zeros(F, bool)
    np.logical_or.at(flagged, i[sure_t], True)
    np.logical_or.at(flagged, j[sure_t], True)
    amb_pair = ~sure_t & ~sure_f
    touched = np.zeros(F, bool)
    np.logical_or.at(touched, i[amb_pair], True)
    np.logical_or.at(touched, j[amb_pair], True)
    ambiguous = touched & ~flagged
    clean = ~flagged & ~ambiguous
    return flagged, clean, ambiguous


def classify_batch(vertices, faces, tol_rel=TOL):
    out = [classify(v, faces, tol_rel) for v in np.asarray(vertices)]
    return tuple(np.stack([o[k] for o in out]) for k in range(3))


# ---- meshes of the tests ---------------------------------------------------------------------------------------------------------------
def torus(n_u=84, n_v=82, R=1.0, r=0.4):
    """Closed torus grid: V = n_u n_v, F = 2 V; r > R gives a self-intersecting spindle torus."""
    u = np.arange(n_u) * (2 * np.pi / n_u)
    v = np.arange(n_v) * (2 * np.pi / n_v)
    U, W = np.meshgrid(u, v, indexing="ij")
    X = np.stack([(R + r * np.cos(W)) * np.cos(U), (R + r * np.cos(W)) * np.sin(U), r * np.sin(W)], -1).reshape(-1, 3)
    ii, jj = np.meshgrid(np.arange(n_u), np.arange(n_v), indexing="ij")
    a = ii * n_v + jj
    b = ((ii + 1) % n_u) * n_v + jj
    c = ((ii + 1) % n_u) * n_v + (jj + 1) % n_v
    d = ii * n_v + (jj + 1) % n_v
    faces = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)])
    return X.astype(np.float32), faces.astype(np.int32)


def smooth_deform(X, seed, amp=0.08):
    """A random smooth displacement field: a few low-frequency sinusoids per axis."""
    rs = np.random.RandomState(seed)
    out = X.astype(np.float64).copy()
    for _ in range(3):
        k = rs.normal(size=3) * 1.5
        ph = rs.uniform(0, 2 * np.pi)
        out += amp * rs.normal(size=3) * np.sin(X.astype(np.float64) @ k + ph)[:, None]
    return out.astype(np.float32)


def hand_cases():
    """name -> (vertices [V, 3], faces [F, 3], expected flags [F]); coordinates chosen so fp32 computes every predicate exactly."""
    f32 = lambda a: np.asarray(a, dtype=np.float32)
    i32 = lambda a: np.asarray(a, dtype=np.int32)
    base = [[0, 0, 0], [4, 0, 0], [0, 4, 0]]                               # in z = 0
    cases = {
        # a vertical triangle through the interior of the base
        "piercing": (f32(base + [[1, 1, -1], [1, 1, 2], [2, 1, 2]]), i32([[0, 1, 2], [3, 4, 5]]), [1, 1]),
        # a vertex of the second on the interior of the first, the rest above
        "touching": (f32(base + [[1, 1, 0], [1, 1, 2], [2, 1, 2]]), i32([[0, 1, 2], [3, 4, 5]]), [1, 1]),
        # clear of each other
        "apart": (f32(base + [[1, 1, 1], [1, 1, 2], [2, 1, 2]]), i32([[0, 1, 2], [3, 4, 5]]), [0, 0]),
        # shared vertex 0; the second folds down through the first: its mid-edge segment crosses the first's interior
        "shared_vertex_piercing": (f32(base + [[4, 2, -1], [2, 4, 1]]), i32([[0, 1, 2], [0, 3, 4]]), [1, 1]),
        # the same pair with the faces in the other order (the swapped direction decides)
        "shared_vertex_piercing_swapped": (f32(base + [[4, 2, -1], [2, 4, 1]]), i32([[0, 3, 4], [0, 1, 2]]), [1, 1]),
        # shared vertex 0, the second leaves the first's plane at once: they meet only at the shared vertex
        "shared_vertex_touching": (f32(base + [[-2, 1, 2], [-1, -2, 2]]), i32([[0, 1, 2], [0, 3, 4]]), [0, 0]),
        # two faces on edge (0, 1) folded flat onto each other: overlap in their plane, but an edge pair is never tested
        "edge_fold_coplanar": (f32(base + [[2, 1, 0]]), i32([[0, 1, 2], [0, 1, 3]]), [0, 0]),
        # coplanar overlap without shared indices
        "coplanar_overlap": (f32(base + [[1, 1, 0], [5, 1, 0], [1, 5, 0]]), i32([[0, 1, 2], [3, 4, 5]]), [1, 1]),
        # the same corners listed twice (and a third face far away)
        "duplicate_face": (f32(base + [[8, 8, 8], [9, 8, 8], [8, 9, 8]]), i32([[0, 1, 2], [2, 0, 1], [3, 4, 5]]), [1, 1, 0]),
        # a face with a repeated index inside a piercing pair: never tested, never flagged
        "degenerate_face": (f32(base + [[1, 1, -1], [1, 1, 2], [2, 1, 2]]), i32([[0, 1, 2], [3, 4, 5], [3, 3, 4]]), [1, 1, 0]),
    }
    return {k: (v, f, np.asarray(e, bool)) for k, (v, f, e) in cases.items()}
