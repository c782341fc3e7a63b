#!/usr/bin/env python3
"""Golden g29_rigid_align: outputs of the reference's own rigid_transform_3D / rigid_align (lib/utils/transforms.py:264-286),
compute_bbox / bbox_from_detector (lib/utils/preprocess.py:117-159) and MocapDataset.eval_EHF (lib/dataset/mocap_dataset.py:61-84),
captured by importing the reference (read-only) -- run in the build container only:

    python tests/golden/gen_golden_align.py

* alignment: the point sets of tests/align_ref.generate_pairs at N = 4, 22, 55 (fp32 values, handed to the reference as fp64) and a few
  hand-built ones (identity, mirrored target, coplanar points, triangles);
* eval_EHF: a MocapDataset made without its __init__ (cv2 / smplx are not installed) with stand-ins: ``smplx`` = an object holding the
  synthetic SMPL-X asset's J_regressor (fp64 copy of the fp32 values) and J_regressor_idx whose call returns the recorded predicted
  vertices (fp64 oracle.fk_torch.smplx_forward, rounded to fp32, handed over as fp64 so that the whole evaluation is fp64 numpy);
  load_ply patched to return the recorded ground-truth mesh; cam_param['R'] from scipy's Rotation.from_rotvec of the reference's vector.
  The meshes are stored only at the vertices the first 22 regressor rows name (every other vertex meets a zero weight).
Arrays only: inputs and the reference's outputs.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))
from gen_golden import _stub_finder, save  # noqa: E402

EHF_ROTVEC = [-2.98747896, 0.01172457, -0.05704687]


def ehf_case(asset, n_images, seed):
    """Predicted / ground-truth meshes of n_images bodies (fp32): random poses and shapes several metres from the origin; the ground truth
    is another pose under a similarity, in the frame the EHF rotation takes to the camera's."""
    sys.path.insert(0, os.path.join(HERE, "..", ".."))
    from oracle import fk_torch
    rs = np.random.RandomState(seed)

    def bodies(scale_pose):
        pose = torch.tensor(rs.standard_normal((n_images, 63)) * scale_pose)
        orient = torch.tensor(rs.standard_normal((n_images, 3)) * 0.5)
        betas = torch.tensor(rs.standard_normal((n_images, asset["num_betas"])) * 0.5)
        transl = torch.tensor(np.stack([rs.uniform(-1, 1, n_images), rs.uniform(-1, 1, n_images), rs.uniform(2, 4, n_images)], 1))
        with torch.no_grad():
            v, _ = fk_torch.smplx_forward(asset, pose, betas=betas, global_orient=orient, transl=transl)
        return v.numpy()

    pred = bodies(0.3).astype(np.float32)
    gt = bodies(0.3)
    from scipy.spatial.transform import Rotation
    for k in range(n_images):
        Rk = Rotation.from_rotvec(rs.standard_normal(3)).as_matrix()
        gt[k] = rs.uniform(0.8, 1.25) * (gt[k] @ Rk.T) + rs.uniform(-3, 3, 3)
    return pred, gt.astype(np.float32)


def main():
    _stub_finder()
    import lib.utils.transforms as ref_tf
    import lib.utils.preprocess as ref_pp
    import lib.dataset.mocap_dataset as ref_md
    import align_ref
    from scipy.spatial.transform import Rotation
    sys.path.insert(0, os.path.join(HERE, "..", ".."))
    from dposer_amd.body_model.synthetic import make_synthetic_smplx_asset

    out = {}
    # ---- rigid_transform_3D / rigid_align
    for n, count, seed in ((4, 40, 2904), (22, 40, 2922), (55, 20, 2955)):
        src, dst, kept, reflected = align_ref.generate_pairs(n, count, seed)
        c, R, t, al = [], [], [], []
        for k in range(count):
            A, B = src[k].astype(np.float64), dst[k].astype(np.float64)
            ck, Rk, tk = ref_tf.rigid_transform_3D(A, B)
            c.append(ck); R.append(Rk); t.append(tk); al.append(ref_tf.rigid_align(A, B))
        out[f"ra{n}_src"], out[f"ra{n}_dst"], out[f"ra{n}_kept"], out[f"ra{n}_reflected"] = src, dst, kept, reflected
        out[f"ra{n}_c"], out[f"ra{n}_R"], out[f"ra{n}_t"], out[f"ra{n}_aligned"] = np.asarray(c), np.stack(R), np.stack(t), np.stack(al)
    rs = np.random.RandomState(2900)
    base = (rs.standard_normal((8, 3)) * [0.4, 0.25, 0.1] + [1.5, -2.0, 3.0]).astype(np.float32)
    Rh = Rotation.from_rotvec([0.3, -1.1, 0.6]).as_matrix()
    sim = (1.3 * base.astype(np.float64) @ Rh.T + [0.5, 2.0, -1.0]).astype(np.float32)
    mirrored = (sim * np.array([1, 1, -1], np.float32)).astype(np.float32)
    plane = base.copy(); plane[:, 2] = 3.0
    plane_dst = (0.8 * plane.astype(np.float64) @ Rh.T + [0.1, 0.2, 0.3] + rs.standard_normal((8, 3)) * 0.01).astype(np.float32)
    tri = np.array([[0.0, 0.0, 2.0], [0.4, 0.1, 2.2], [0.1, 0.5, 1.9]], np.float32)
    tri_dst = (1.1 * tri.astype(np.float64) @ Rh.T + [1.0, -1.0, 0.5]).astype(np.float32)
    tri2 = np.array([[1.0, 2.0, 3.0], [1.3, 2.0, 3.1], [1.0, 2.6, 2.8]], np.float32)
    tri2_dst = (0.9 * tri2.astype(np.float64) @ Rh + [-2.0, 0.3, 0.0] + rs.standard_normal((3, 3)) * 0.02).astype(np.float32)
    hand = {"identity": (base, base), "similarity": (base, sim), "mirrored": (base, mirrored), "coplanar": (plane, plane_dst),
            "triangle": (tri, tri_dst), "triangle2": (tri2, tri2_dst)}
    for name, (A, B) in hand.items():
        ck, Rk, tk = ref_tf.rigid_transform_3D(A.astype(np.float64), B.astype(np.float64))
        out[f"hand_{name}_src"], out[f"hand_{name}_dst"] = A, B
        out[f"hand_{name}_c"], out[f"hand_{name}_R"], out[f"hand_{name}_t"] = np.float64(ck), Rk, tk
        out[f"hand_{name}_aligned"] = ref_tf.rigid_align(A.astype(np.float64), B.astype(np.float64))
    out["hand_names"] = np.array(list(hand))

    # ---- compute_bbox / bbox_from_detector
    kp = rs.uniform(50, 900, (4, 25, 3))
    kp[:, :, 2] = rs.uniform(0.05, 1.0, (4, 25))
    kp[0, rs.choice(25, 9, replace=False), 2] = 0.0
    kp[2, :, 2] = 0.0                                                   # a person with no visible keypoint: skipped
    kp[3, :20, 2] = 0.0
    json_data = {"people": [{"pose_keypoints_2d": p.reshape(-1).tolist()} for p in kp]}
    out["bbox_keypoints"] = kp
    out["bbox_out"] = ref_pp.compute_bbox(json_data)
    boxes = np.array([[400.0, 100.0, 1000.0, 1200.0], [10.5, 20.25, 300.0, 180.0], [0.0, 0.0, 64.0, 512.0]])
    cen, sc = [], []
    for bb, rescale in zip(boxes, (1.1, 1.1, 1.25)):
        c_, s_ = ref_pp.bbox_from_detector(torch.tensor(bb), rescale)
        assert c_.dtype == torch.float64
        cen.append(c_.numpy()); sc.append(float(s_))
    out["bfd_boxes"], out["bfd_rescale"] = boxes, np.array([1.1, 1.1, 1.25])
    out["bfd_center"], out["bfd_scale"] = np.stack(cen), np.asarray(sc, np.float64)

    # ---- MocapDataset.eval_EHF
    asset = make_synthetic_smplx_asset(seed=0)
    J = asset["J_regressor"]
    used = np.flatnonzero((J[:22] != 0).any(0)).astype(np.int32)
    n_images = 6
    pred, gt = ehf_case(asset, n_images, 2929)
    db = object.__new__(ref_md.MocapDataset)
    db.cam_param = {"R": Rotation.from_rotvec(EHF_ROTVEC).as_matrix()}
    pa, mp = [], []

    class SmplxStandIn:
        J_regressor = J.astype(np.float64)
        J_regressor_idx = {"pelvis": 0}

        def __init__(self, vertices):
            self.vertices = vertices

        def __call__(self, betas=None, pose_body=None, root_orient=None, trans=None):
            return types.SimpleNamespace(v=torch.tensor(self.vertices[None].astype(np.float64)))

    for k in range(n_images):
        db.smplx = SmplxStandIn(pred[k])
        ref_md.load_ply = lambda path, k=k: gt[k].astype(np.float64)
        res = db.eval_EHF((torch.zeros(1, 66), torch.zeros(1, 10), torch.zeros(1, 3), None), "unused.ply")
        pa.append(res["pa_mpjpe_body"][0]); mp.append(res["mpjpe_body"][0])
    out["ehf_used_vertices"], out["ehf_pred_used"], out["ehf_gt_used"] = used, pred[:, used], gt[:, used]
    out["ehf_rotation"] = db.cam_param["R"]
    out["ehf_rotvec"] = np.asarray(EHF_ROTVEC)
    out["ehf_pa_mpjpe"], out["ehf_mpjpe"] = np.asarray(pa, np.float64), np.asarray(mp, np.float64)
    save("g29_rigid_align", **out)


if __name__ == "__main__":
    main()
