"""fp64 numpy statement of the rules of include/dposer_hip.h for dposer_rigid_align, dposer_regress_joints and dposer_ehf_eval, and
the generator of the point sets the alignment tests run on.  Pinned to the reference's own outputs (tests/golden/g29_rigid_align.npz)
by tests/test_rigid_align_cpu.py before anything on the GPU is compared with it."""
import numpy as np

CONDITION_GATE = 1e-2          # sets with (s2 + s3) / s1 of H below this are left out (the polar factor is ill-conditioned there)


def _cross_covariance(A, B):
    A = np.asarray(A, np.float64)
    B = np.asarray(B, np.float64)
    ma, mb = A.mean(0), B.mean(0)
    return (A - ma).T @ (B - mb) / A.shape[0], ma, mb


def similarity(A, B):
    """(c, R, t) taking the points A [N, 3] onto B [N, 3]: R = V U^T of H = U S V^T (proper: the last singular value and right vector
    change sign when det < 0), c = sum(s) / total population variance of A, t = mean(B) - c R mean(A)."""
    H, ma, mb = _cross_covariance(A, B)
    U, s, Vt = np.linalg.svd(H)
    s = s.copy()
    Vt = Vt.copy()
    R = Vt.T @ U.T
    if np.linalg.det(R) < 0:
        s[2] = -s[2]
        Vt[2] = -Vt[2]
        R = Vt.T @ U.T
    with np.errstate(divide="ignore", invalid="ignore"):
        c = s.sum() / np.asarray(A, np.float64).var(0).sum()
    return c, R, mb - c * (R @ ma)


def align(A, B):
    c, R, t = similarity(A, B)
    return c * (np.asarray(A, np.float64) @ R.T) + t


def mean_distance(P, Q):
    return np.sqrt(((np.asarray(P, np.float64) - np.asarray(Q, np.float64)) ** 2).sum(-1)).mean(-1)


def takes_reflection_branch(A, B):
    H, _, _ = _cross_covariance(A, B)
    U, _, Vt = np.linalg.svd(H)
    return np.linalg.det(Vt.T @ U.T) < 0


def conditioning(A, B):
    """(s2 + s3) / s1 of H, s3 counted negative where the reflection branch is taken."""
    H, _, _ = _cross_covariance(A, B)
    s = np.linalg.svd(H, compute_uv=False)
    s3 = -s[2] if takes_reflection_branch(A, B) else s[2]
    return (s[1] + s3) / s[0] if s[0] > 0 else 0.0


def regress(W, vertices, rows=22):
    """joints [..., rows, 3] = W[:rows] @ vertices [..., V, 3] in fp64 (W dense or scipy-sparse)."""
    W = np.asarray(W.todense() if hasattr(W, "todense") else W, np.float64)[:rows]
    return np.einsum("rv,...vk->...rk", W, np.asarray(vertices, np.float64))


def ehf_metrics(W, pred_vertices, gt_vertices, rotation=None, pelvis=0, rows=22):
    """(pa_mpjpe, mpjpe) in millimetres of one image: the joints of both meshes, the ground truth rotated, the prediction aligned."""
    jp = regress(W, pred_vertices, rows)
    jg = regress(W, gt_vertices, rows)
    if rotation is not None:
        jg = jg @ np.asarray(rotation, np.float64).T
    pa = mean_distance(align(jp, jg), jg) * 1000
    mp = mean_distance(jp - jp[pelvis] + jg[pelvis], jg) * 1000
    return pa, mp


def _random_rotation(rs):
    q = rs.standard_normal(4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def generate_pairs(n_points, count, seed):
    """Body-sized test pairs, fp32: an anisotropic Gaussian cloud (sigmas 0.35-0.5, 0.2-0.3 and 0.08-0.15 m along three random
    orthogonal axes -- the proportions of a standing body; distinct axes keep s2 away from s3, which is what conditions a mirrored
    target), the target a random similarity of it (scale 0.7-1.4) plus 3 cm noise, every fourth target mirrored, both sets displaced by
    up to 4 m per axis.
    Returns (src [count, N, 3], dst, kept [count] bool: conditioning >= CONDITION_GATE, reflected [count] bool)."""
    rs = np.random.RandomState(seed)
    src = np.empty((count, n_points, 3), np.float32)
    dst = np.empty((count, n_points, 3), np.float32)
    kept = np.zeros(count, bool)
    reflected = np.zeros(count, bool)
    for k in range(count):
        sig = np.array([rs.uniform(0.35, 0.5), rs.uniform(0.2, 0.3), rs.uniform(0.08, 0.15)])
        A = (rs.standard_normal((n_points, 3)) * sig) @ _random_rotation(rs).T
        Bp = rs.uniform(0.7, 1.4) * (A @ _random_rotation(rs).T)
        if k % 4 == 3:
            Bp = Bp * np.array([1.0, 1.0, -1.0])
        Bp = Bp + rs.standard_normal((n_points, 3)) * 0.03
        src[k] = A + rs.uniform(-4, 4, 3)
        dst[k] = Bp + rs.uniform(-4, 4, 3)
        kept[k] = conditioning(src[k], dst[k]) >= CONDITION_GATE
        reflected[k] = takes_reflection_branch(src[k], dst[k])
    return src, dst, kept, reflected


def kept_pairs(n_points, count, seed):
    """The pairs of generate_pairs that pass the conditioning gate, with the caps on what the gate may drop asserted: at most 2 % of a
    size, nothing at N >= 22, and at least a fifth of the kept sets on the det R < 0 branch."""
    src, dst, kept, reflected = generate_pairs(n_points, count, seed)
    dropped = int((~kept).sum())
    assert dropped <= 0.02 * count, (n_points, dropped, count)
    if n_points >= 22:
        assert dropped == 0, (n_points, dropped)
    assert reflected[kept].mean() >= 0.2, (n_points, reflected[kept].mean())
    return src[kept], dst[kept]


def write_ply(path, vertices, fmt="binary_little_endian", dtype="float", extra=(), faces=None, faces_first=False):
    """A PLY file of ``vertices`` [V, 3] for the reader's tests: ``extra`` = [(name, ply type, column)] more vertex properties (written
    after x, y, z), ``faces`` an optional list element (uchar count, int indices) before or after the vertex element."""
    np_of = {"float": "f4", "double": "f8", "uchar": "u1", "int": "i4", "short": "i2"}
    order = {"ascii": "=", "binary_little_endian": "<", "binary_big_endian": ">"}[fmt]
    V = np.asarray(vertices)
    props = [("x", dtype, V[:, 0]), ("y", dtype, V[:, 1]), ("z", dtype, V[:, 2])] + list(extra)
    vert_hdr = [f"element vertex {len(V)}"] + [f"property {t} {n}" for n, t, _ in props]
    face_hdr = [f"element face {len(faces)}", "property list uchar int vertex_indices"] if faces is not None else []
    hdr = ["ply", f"format {fmt} 1.0", "comment written by the tests"] + (face_hdr + vert_hdr if faces_first else vert_hdr + face_hdr) + ["end_header"]

    def vert_body():
        if fmt == "ascii":
            return "".join(" ".join(repr(float(c[i])) if np_of[t][0] == "f" else str(int(c[i])) for _, t, c in props) + "\n"
                           for i in range(len(V))).encode()
        rec = np.empty(len(V), dtype=[(n, order + np_of[t]) for n, t, _ in props])
        for n, _, c in props:
            rec[n] = c
        return rec.tobytes()

    def face_body():
        if faces is None:
            return b""
        if fmt == "ascii":
            return "".join(f"{len(f)} " + " ".join(str(int(i)) for i in f) + "\n" for f in faces).encode()
        return b"".join(np.uint8(len(f)).tobytes() + np.asarray(f, dtype=order + "i4").tobytes() for f in faces)

    with open(path, "wb") as fh:
        fh.write(("\n".join(hdr) + "\n").encode("ascii"))
        fh.write(face_body() + vert_body() if faces_first else vert_body() + face_body())
