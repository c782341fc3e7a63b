"""Generation metrics (reference lib/utils/metric.py).

``average_pairwise_distance`` is the APD of run/demo.py's ``--metrics`` path.  The reference fills a [B, B] matrix with
a Python double loop (B^2/2 tiny kernels); here it is one batched distance computation on whatever device the joints
live on, chunked so the [chunk, B, J] intermediate stays bounded.

``self_intersecting_faces`` / ``self_intersections_percentage_hip`` are the SI metric computed by this package's own kernels
(csrc/meshsi.hip, pair rule in include/dposer_hip.h); ``self_intersections_percentage`` stays the reference's PyMeshLab path.
``generation_metrics`` is the APD + SI pair of demo.py:148-161.

``pose_set_distances`` and what is built on it (``average_pairwise_distance_hip``, ``nearest_pose_distance``, ``generation_fidelity``) reduce
over the matrix of APD distances between two pose sets without storing it (csrc/setdist.hip, rules in include/dposer_hip.h)."""
import ctypes as C

import numpy as np
import torch


def average_pairwise_distance(joints3d, chunk=1024):
    """APD of ``joints3d [B, J, 3]`` (metric.py:8-37): mean over ordered pairs i != j of the mean per-joint Euclidean
    distance between poses i and j."""
    B = joints3d.shape[0]
    x = joints3d.float()
    total = torch.zeros((), dtype=torch.float64, device=x.device)
    for lo in range(0, B, chunk):
        d = torch.linalg.norm(x[lo:lo + chunk, None] - x[None], dim=-1).mean(dim=-1)      # [c, B]; the diagonal is exactly 0
        total += d.double().sum()
    return (total / (B * (B - 1))).float()


MAX_NEIGHBOURS, MAX_SET_JOINTS = 8, 128          # limits of dposer_pose_set_distances


def _pose_set(x, name):
    if not isinstance(x, torch.Tensor) or x.dim() != 3 or x.shape[-1] != 3:
        raise ValueError(f"{name} must be a tensor [N, J, 3], got {tuple(x.shape) if hasattr(x, 'shape') else type(x).__name__}")
    if x.shape[0] < 1 or not 1 <= x.shape[1] <= MAX_SET_JOINTS:
        raise ValueError(f"{name} needs N >= 1 poses of 1 <= J <= {MAX_SET_JOINTS} joints, got {tuple(x.shape)}")
    return x


def pose_set_distances(a, b=None, *, k=0, radii=None, want_sum=False, splits=0):
    """Reductions over the distances d(a_i, b_j) = mean over joints of ||a_i - b_j|| of two pose sets ``a [na, J, 3]`` and ``b [nb, J, 3]`` on a ROCm
    device (``dposer_pose_set_distances``; the rules are written out in include/dposer_hip.h).  ``b=None``: the set against itself, each
    row's own index left out of the neighbour and covered outputs.  Returns a dict of device tensors with, as asked for,
    ``"knn_dist" float32 [na, k]`` / ``"knn_idx" int32 [na, k]`` (``1 <= k <= 8``: the k nearest, ascending, ties to the smaller index, tail
    ``+inf`` / ``-1``), ``"covered" int32 [na]`` (``radii float [nb]`` given: the count of j with d(a_i, b_j) <= radii[j]) and ``"sum"
    float64 []`` (``want_sum``: the sum of all distances).  ``splits``: 0 = the library's choice; the outputs do not depend on it beyond the
    last bits of ``sum``.  Never synchronises with the host."""
    from .. import _C
    a = _pose_set(a, "a")
    same = b is None
    if not same:
        b = _pose_set(b, "b")
        if b.shape[1] != a.shape[1]:
            raise ValueError(f"a and b must have the same joint count, got {a.shape[1]} and {b.shape[1]}")
    na, J = int(a.shape[0]), int(a.shape[1])
    nb = na if same else int(b.shape[0])
    k, splits = int(k), int(splits)
    if not 0 <= k <= MAX_NEIGHBOURS:
        raise ValueError(f"k must lie in [0, {MAX_NEIGHBOURS}], got {k}")
    if splits < 0:
        raise ValueError(f"splits must be >= 0, got {splits}")
    if nb >= 2 ** 31:
        raise ValueError("reference sets of 2^31 poses and more are not supported")
    if radii is not None and (not isinstance(radii, torch.Tensor) or tuple(radii.shape) != (nb,)):
        raise ValueError(f"radii must be a tensor [{nb}], got {tuple(radii.shape) if hasattr(radii, 'shape') else type(radii).__name__}")
    if k == 0 and radii is None and not want_sum:
        raise ValueError("nothing asked for: give k >= 1, radii or want_sum=True")
    _C.require_gpu(a, "a")
    if not same:
        _C.require_gpu(b, "b")
    if radii is not None:
        _C.require_gpu(radii, "radii")
    dev = a.device
    a = a.detach().to(torch.float32).contiguous()
    b = None if same else b.detach().to(device=dev, dtype=torch.float32).contiguous()
    radii = None if radii is None else radii.detach().to(device=dev, dtype=torch.float32).contiguous()
    out = {}
    if k > 0:
        out["knn_dist"] = torch.empty((na, k), dtype=torch.float32, device=dev)
        out["knn_idx"] = torch.empty((na, k), dtype=torch.int32, device=dev)
    if radii is not None:
        out["covered"] = torch.empty((na,), dtype=torch.int32, device=dev)
    if want_sum:
        out["sum"] = torch.empty((), dtype=torch.float64, device=dev)
    lib = _C.lib()
    nbytes = int(lib.dposer_pose_set_distances_scratch_bytes(na, nb, J, k, splits))
    if nbytes < 0:
        _C.check(nbytes, "dposer_pose_set_distances_scratch_bytes")
    scratch = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    args = _C.SetDistArgs(a=a.data_ptr(), b=None if same else b.data_ptr(), na=na, nb=nb, joints=J, same_set=1 if same else 0, k=k,
                          radii=None if radii is None else radii.data_ptr(), sum=out["sum"].data_ptr() if want_sum else None,
                          knn_dist=out["knn_dist"].data_ptr() if k > 0 else None, knn_idx=out["knn_idx"].data_ptr() if k > 0 else None,
                          covered=out["covered"].data_ptr() if radii is not None else None, splits=splits, scratch=scratch.data_ptr())
    with torch.cuda.device(dev):
        _C.check(lib.dposer_pose_set_distances(C.byref(args), _C.stream_ptr()), "dposer_pose_set_distances")
    return out


def average_pairwise_distance_hip(joints3d):
    """APD of ``joints3d [B, J, 3]`` as a device scalar (float32), the quantity of ``average_pairwise_distance`` without its
    ``[chunk, B, J, 3]`` intermediate: one ``pose_set_distances`` call in its symmetric form."""
    B = int(joints3d.shape[0]) if hasattr(joints3d, "shape") and len(joints3d.shape) else 0
    if B < 2:
        raise ValueError("APD needs at least two poses")
    total = pose_set_distances(joints3d, want_sum=True)["sum"]
    return (total / (B * (B - 1))).float()


def nearest_pose_distance(query, reference, k=1):
    """``(dist float32 [N, k], idx int32 [N, k])``: the ``k`` nearest poses of ``reference [M, J, 3]`` to each pose of ``query [N, J, 3]``
    under the APD distance, ascending (the memorisation / novelty check of a generated set against the training set)."""
    if int(k) < 1:
        raise ValueError(f"k must be >= 1, got {k}")
    out = pose_set_distances(query, reference, k=k)
    return out["knn_dist"], out["knn_idx"]


def generation_fidelity(gen_joints, real_joints, k=3):
    """Fidelity scores of generated poses ``G = gen_joints [N, J, 3]`` against real ones ``R = real_joints [M, J, 3]`` under the APD
    distance, as device scalars: ``{"APD", "dNN", "precision", "recall", "density", "coverage"}``.

    With r_R[i] the distance of R_i to its k-th nearest neighbour inside R (itself excluded) and r_G[n] the same inside G:
    ``precision`` = mean_n 1[exists i: d(G_n, R_i) <= r_R[i]] and ``recall`` = mean_i 1[exists n: d(R_i, G_n) <= r_G[n]] (improved
    precision / recall, Kynkaanniemi et al. 2019); ``density`` = sum_n #{i: d(G_n, R_i) <= r_R[i]} / (k N) and ``coverage`` =
    mean_i 1[min_n d(R_i, G_n) <= r_R[i]] (Naeem et al. 2020); ``dNN`` = mean_n min_i d(G_n, R_i); ``APD`` of G.  Five library calls:
    the radii of R and of G, G against R (covered + nearest), R against G (covered + nearest), and the APD sum.  Needs N, M >= k + 1."""
    gen_joints, real_joints = _pose_set(gen_joints, "gen_joints"), _pose_set(real_joints, "real_joints")
    k = int(k)
    if not 1 <= k <= MAX_NEIGHBOURS:
        raise ValueError(f"k must lie in [1, {MAX_NEIGHBOURS}], got {k}")
    if gen_joints.shape[1] != real_joints.shape[1]:
        raise ValueError(f"both sets must have the same joint count, got {gen_joints.shape[1]} and {real_joints.shape[1]}")
    N, M = int(gen_joints.shape[0]), int(real_joints.shape[0])
    if N < k + 1 or M < k + 1:
        raise ValueError(f"generation_fidelity with k = {k} needs at least {k + 1} poses in each set, got {N} and {M}")
    r_real = pose_set_distances(real_joints, k=k)["knn_dist"][:, k - 1].contiguous()
    r_gen = pose_set_distances(gen_joints, k=k)["knn_dist"][:, k - 1].contiguous()
    g2r = pose_set_distances(gen_joints, real_joints, k=1, radii=r_real)
    r2g = pose_set_distances(real_joints, gen_joints, k=1, radii=r_gen)
    apd = average_pairwise_distance_hip(gen_joints)
    cov_g, cov_r = g2r["covered"], r2g["covered"]
    return {"APD": apd,
            "dNN": g2r["knn_dist"][:, 0].double().mean().float(),
            "precision": (cov_g > 0).double().mean().float(),
            "recall": (cov_r > 0).double().mean().float(),
            "density": (cov_g.double().sum() / (k * N)).float(),
            "coverage": (r2g["knn_dist"][:, 0] <= r_real).double().mean().float()}


def self_intersections_percentage(vertices, faces):
    """Percentage of self-intersecting faces per mesh (metric.py:41-92).  The reference delegates to PyMeshLab and returns
    NaNs when it is not importable; PyMeshLab is not part of this image, so this always takes that branch."""
    try:
        import pymeshlab as pyml
    except ImportError:
        return np.ones(len(vertices)) * np.nan
    if isinstance(vertices, torch.Tensor):
        vertices = vertices.detach().cpu().numpy()
    if isinstance(faces, torch.Tensor):
        faces = faces.detach().cpu().numpy()
    out = np.zeros(len(vertices))
    for i, v in enumerate(vertices):
        ms = pyml.MeshSet()
        ms.add_mesh(pyml.Mesh(v, faces))
        n_all = ms.get_topological_measures()["faces_number"]
        ms.compute_selection_by_self_intersections_per_face()
        ms.meshing_remove_selected_faces()
        out[i] = (n_all - ms.get_topological_measures()["faces_number"]) / n_all * 100
    return out


def _morton_face_order(vertices0, faces):
    """A face order in which runs of 64 consecutive faces are compact patches: Morton (Z-order) rank of the face centroids of one
    mesh, 10 bits per axis.  Surface adjacency does not change with pose, so the order of mesh 0 keeps tiles tight in every mesh."""
    c = vertices0[faces].mean(dim=1).nan_to_num(0.0, 0.0, 0.0)                          # [F, 3]
    lo, hi = c.min(dim=0).values, c.max(dim=0).values
    q = ((c - lo) / (hi - lo).clamp_min(1e-30) * 1023.0).round().clamp(0, 1023).to(torch.int64)
    code = torch.zeros(len(faces), dtype=torch.int64, device=faces.device)
    for bit in range(10):
        for axis in range(3):
            code |= ((q[:, axis] >> bit) & 1) << (3 * bit + axis)
    return torch.argsort(code, stable=True).to(torch.int32)


def _mesh_si(vertices, faces):
    """(flags uint8 [B, F], counts int32 [B]) of dposer_mesh_self_intersections."""
    from .. import _C
    if vertices.dim() != 3 or vertices.shape[-1] != 3:
        raise ValueError(f"vertices must be [B, V, 3], got {tuple(vertices.shape)}")
    if faces.dim() != 2 or faces.shape[-1] != 3:
        raise ValueError(f"faces must be [F, 3], got {tuple(faces.shape)}")
    _C.require_gpu(vertices, "vertices")
    _C.require_gpu(faces, "faces")
    B, V, F = int(vertices.shape[0]), int(vertices.shape[1]), int(faces.shape[0])
    if F == 0:
        raise ValueError("faces is empty: the self-intersection percentage of a mesh without faces is undefined")
    if faces.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"faces must hold int32 or int64 vertex indices, got {faces.dtype}")
    if V >= 2 ** 31 or F >= 2 ** 31:
        raise ValueError("meshes of 2^31 vertices or faces and more are not supported")
    dev = vertices.device
    flags = torch.zeros((B, F), dtype=torch.uint8, device=dev)
    counts = torch.zeros((B,), dtype=torch.int32, device=dev)
    if B == 0:
        return flags, counts
    lo, hi = int(faces.min()), int(faces.max())
    if lo < 0 or hi >= V:
        raise ValueError(f"face indices must lie in [0, {V}), got [{lo}, {hi}]")
    f32 = faces.to(device=dev, dtype=torch.int32).contiguous()                        # (int64 faces: converted once)
    v = vertices.detach().to(torch.float32).contiguous()
    order = _morton_face_order(v[0], f32.long())
    l = _C.lib()
    tiles = -(-F // 64)
    group = max(1, (1 << 26) // tiles)                # grid limit of one call: batch x tiles <= 2^26 waves (meshes are independent)
    scratch = torch.empty((int(l.dposer_mesh_self_intersections_scratch_bytes(min(B, group), F)),), dtype=torch.uint8, device=dev)
    for g0 in range(0, B, group):
        nb = min(group, B - g0)
        a = _C.MeshSiArgs(vertices=v[g0].data_ptr(), batch=nb, num_vertices=V, faces=f32.data_ptr(), num_faces=F,
                          face_order=order.data_ptr(), flags=flags[g0].data_ptr(), counts=counts[g0:].data_ptr(),
                          scratch=scratch.data_ptr())
        _C.check(l.dposer_mesh_self_intersections(C.byref(a), _C.stream_ptr()), "dposer_mesh_self_intersections")
    return flags, counts


def self_intersecting_faces(vertices, faces):
    """``torch.bool [B, F]``: which faces of each mesh ``vertices [B, V, 3]`` (one shared ``faces [F, 3]``) intersect another face
    of the same mesh, under the pair rule of include/dposer_hip.h (dposer_mesh_self_intersections).  ROCm tensors only."""
    return _mesh_si(vertices, faces)[0].bool()


def self_intersections_percentage_hip(vertices, faces):
    """SI per mesh, ``np.ndarray float64 [B]``: 100 x (flagged faces) / F, the quantity of ``self_intersections_percentage``
    computed by the package's kernels instead of PyMeshLab."""
    F = int(faces.shape[0]) if hasattr(faces, "shape") else len(faces)
    counts = _mesh_si(vertices, faces)[1].cpu().numpy().astype(np.float64)
    return counts / F * 100


class IndexList:
    """A vertex / joint-row list of ``pose_pair_errors`` checked on the host once: ``host`` (int32 numpy), its length ``n`` and largest
    entry ``max``, and one int32 device copy per device (``on(device)``)."""

    def __init__(self, idx, limit, name="index list"):
        if isinstance(idx, torch.Tensor):
            idx = idx.detach().cpu().numpy()
        arr = np.asarray(idx)
        if arr.ndim != 1 or arr.size < 1:
            raise ValueError(f"{name} must be a non-empty 1-D list of indices, got shape {arr.shape}")
        if not np.issubdtype(arr.dtype, np.integer):
            raise ValueError(f"{name} must hold integers, got {arr.dtype}")
        lo, hi = int(arr.min()), int(arr.max())
        if lo < 0 or hi >= limit:
            raise ValueError(f"{name} entries must lie in [0, {limit}), got [{lo}, {hi}]")
        self.host = np.ascontiguousarray(arr, dtype=np.int32)
        self.n, self.max, self.limit = int(arr.size), hi, int(limit)
        self._dev = {}

    def on(self, device):
        key = str(device)
        t = self._dev.get(key)
        if t is None:
            t = self._dev[key] = torch.tensor(self.host, dtype=torch.int32, device=device)
        return t


def _as_index_list(idx, limit, name):
    if idx is None:
        return None
    if isinstance(idx, IndexList):
        if idx.limit != limit:
            raise ValueError(f"{name} was checked against {idx.limit} entries, this body model has {limit}")
        return idx
    return IndexList(idx, limit, name)


def _score_fronts(core, ref, hyp, hg, verts, rows, scale, min_into, mpvpe, mpjpe, mpvpe_h=None, mpjpe_h=None):
    """One ``dposer_pose_pair_errors`` call on two ``lbs_front`` results: ``ref`` of B poses, ``hyp`` of B x ``hg`` (row b * hg + h)."""
    from .. import _C
    lib, h, dev, B = _C.lib(), core._handle(), mpvpe.device, ref.batch
    n_list = verts.n if verts is not None else 0
    scratch = torch.empty(lib.dposer_pose_pair_errors_scratch_bytes(h, B, hg, n_list), dtype=torch.uint8, device=dev)
    a = _C.PosePairErrorsArgs(
        body=h, ws_ref=ref.ws.data_ptr(), ws_hyp=hyp.ws.data_ptr(), joints_ref=ref.joints.data_ptr(), joints_hyp=hyp.joints.data_ptr(),
        v_shaped=ref.v_shaped.data_ptr(), v_shaped_batched=1 if ref.batched else 0, skin_k=int(core.skin_idx.shape[1]),
        skin_idx=core.skin_idx.data_ptr(), skin_w=core.skin_w.data_ptr(), transl_ref=None, transl_hyp=None,
        vert_list=None if verts is None else verts.on(dev).data_ptr(), joint_rows=None if rows is None else rows.on(dev).data_ptr(),
        num_listed_vertices=n_list, num_listed_rows=rows.n if rows is not None else 0, max_listed_row=rows.max if rows is not None else 0,
        hypotheses=hg, extra_vertex_ids=core.extra_vertex_ids.data_ptr() if core.n_extra else None,
        lmk_tri=core.lmk_tri.data_ptr() if core.n_lmk else None, lmk_bary=core.lmk_bary_coords.data_ptr() if core.n_lmk else None,
        batch=B, scale=float(scale), min_into=1 if min_into else 0, mpvpe=mpvpe.data_ptr(), mpjpe=mpjpe.data_ptr(),
        mpvpe_h=None if mpvpe_h is None else mpvpe_h.data_ptr(), mpjpe_h=None if mpjpe_h is None else mpjpe_h.data_ptr(), scratch=scratch.data_ptr())
    _C.check(lib.dposer_pose_pair_errors(C.byref(a), _C.stream_ptr()), "dposer_pose_pair_errors")


def pose_pair_errors(body_model, ref_pose_body, hyp_pose_body, *, vert_idx=None, joint_idx=None, scale=1.0, betas=None, per_hypothesis=False,
                     max_workspace_bytes=1 << 30):
    """MPVPE / MPJPE of hypothesis bodies against reference bodies, minimum over the hypotheses, without a vertex tensor
    (``dposer_pose_pair_errors``; the rule is written out in include/dposer_hip.h).

    ``ref_pose_body [B, 63]``, ``hyp_pose_body [B, 63]`` or ``[B, H, 63]`` axis-angle body poses on a ROCm device; ``betas [B, nb]``
    per sample (shared by its hypotheses) or None.  ``vert_idx`` / ``joint_idx``: the vertices and the rows of the LBS joint output to
    average over (None = all) -- host indices (list, numpy, CPU tensor) or an ``IndexList``; they are range-checked on the host, so pass an
    ``IndexList`` built once to keep a device-resident list from being copied back.  ``scale``: 1000 for millimetres.
    Returns ``{"mpvpe": [B], "mpjpe": [B]}`` (+ ``"mpvpe_h"``, ``"mpjpe_h"`` ``[B, H]`` with ``per_hypothesis``) as device tensors.
    One front call (FK + pose-blend offsets) for the references, one per group of hypotheses whose front workspace fits
    ``max_workspace_bytes``; later groups fold into the minimum on the device.  Never synchronises with the host."""
    from .. import _C
    core = getattr(body_model, "bm", body_model)
    n_rows = core.J + core.n_extra + core.n_lmk
    verts = _as_index_list(vert_idx, core.V, "vert_idx")          # (host checks first: they need no device)
    rows = _as_index_list(joint_idx, n_rows, "joint_idx")
    _C.require_gpu(ref_pose_body, "ref_pose_body")
    _C.require_gpu(hyp_pose_body, "hyp_pose_body")
    if hyp_pose_body.dim() == 2:
        hyp_pose_body = hyp_pose_body[:, None]
    if ref_pose_body.dim() != 2 or hyp_pose_body.dim() != 3 or hyp_pose_body.shape[0] != ref_pose_body.shape[0] or \
            hyp_pose_body.shape[2] != ref_pose_body.shape[1]:
        raise ValueError(f"expected ref [B, D] and hyp [B, D] or [B, H, D], got {tuple(ref_pose_body.shape)} and {tuple(hyp_pose_body.shape)}")
    B, H = int(hyp_pose_body.shape[0]), int(hyp_pose_body.shape[1])
    if B < 1 or H < 1:
        raise ValueError("pose_pair_errors needs at least one sample and one hypothesis")
    dev = ref_pose_body.device
    lib, h = _C.lib(), core._handle()
    with torch.no_grad():
        rest = core.rest_shape(betas, None)
        ref = core.lbs_front(rest=rest, body_pose=ref_pose_body)
        # hypotheses per front call: the most whose workspace fits the budget
        group = H
        while group > 1 and lib.dposer_lbs_workspace_bytes(h, B * group) > max_workspace_bytes:
            group -= 1
        rest_h = rest
        out = {"mpvpe": torch.empty(B, dtype=torch.float32, device=dev), "mpjpe": torch.empty(B, dtype=torch.float32, device=dev)}
        per = {"mpvpe_h": [], "mpjpe_h": []}
        for g0 in range(0, H, group):
            hg = min(group, H - g0)
            if rest[2]:                                      # per-sample rest joints, one row per (sample, hypothesis)
                rest_h = (rest[0], rest[1].repeat_interleave(hg, dim=0), True)
            hyp = core.lbs_front(rest=rest_h, body_pose=hyp_pose_body[:, g0:g0 + hg].reshape(B * hg, -1))
            vh = torch.empty(B, hg, dtype=torch.float32, device=dev) if per_hypothesis else None
            jh = torch.empty(B, hg, dtype=torch.float32, device=dev) if per_hypothesis else None
            _score_fronts(core, ref, hyp, hg, verts, rows, scale, g0 > 0, out["mpvpe"], out["mpjpe"], vh, jh)
            hyp = None                                       # (the next group's workspace takes this one's place, not a third)
            if per_hypothesis:
                per["mpvpe_h"].append(vh)
                per["mpjpe_h"].append(jh)
        if per_hypothesis:
            out.update({k: v[0] if len(v) == 1 else torch.cat(v, dim=1) for k, v in per.items()})
    return out


def generation_metrics(body_out):
    """{"APD", "SI"} of demo.py:148-161 from ``BodyModel.forward``'s output (dict or attribute struct): APD over the first 22 joints,
    SI as the mean over the meshes of ``self_intersections_percentage_hip``."""
    get = (lambda k: body_out[k]) if isinstance(body_out, dict) else (lambda k: getattr(body_out, k))
    joints3d, verts, faces = get("Jtr"), get("v"), get("f")
    apd = average_pairwise_distance(joints3d[:, :22, :])
    si = self_intersections_percentage_hip(verts, faces).mean().item()
    return {"APD": apd, "SI": si}
