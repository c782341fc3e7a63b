"""Generation metrics (reference lib/utils/metric.py).

``average_pairwise_distance`` is the APD of run/demo.py's ``--metrics`` path.  The reference fills a [B, B] matrix with
a Python double loop (B^2/2 tiny kernels); here it is one batched distance computation on whatever device the joints
live on, chunked so the [chunk, B, J] intermediate stays bounded.

``self_intersecting_faces`` / ``self_intersections_percentage_hip`` are the SI metric computed by this package's own kernels
(csrc/meshsi.hip, pair rule in include/dposer_hip.h); ``self_intersections_percentage`` stays the reference's PyMeshLab path.
``generation_metrics`` is the APD + SI pair of demo.py:148-161."""
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


def generation_metrics(body_out):
    """{"APD", "SI"} of demo.py:148-161 from ``BodyModel.forward``'s output (dict or attribute struct): APD over the first 22 joints,
    SI as the mean over the meshes of ``self_intersections_percentage_hip``."""
    get = (lambda k: body_out[k]) if isinstance(body_out, dict) else (lambda k: getattr(body_out, k))
    joints3d, verts, faces = get("Jtr"), get("v"), get("f")
    apd = average_pairwise_distance(joints3d[:, :22, :])
    si = self_intersections_percentage_hip(verts, faces).mean().item()
    return {"APD": apd, "SI": si}
