"""Counterpart of the reference's lib/dataset/mocap_dataset.py: ``MocapDataset`` with ``__getitem__`` (the keys run/fitting.py and
run/demo_fit.py read), ``eval_EHF`` (:61-84) and ``print_eval_result`` (:86-88).  The evaluation is one HIP call for B images
(dposer_ehf_eval): joint regression of both meshes, the EHF camera rotation, similarity alignment, PA-MPJPE and pelvis-aligned MPJPE.
``eval_EHF_batch`` is the batched, device-side form; ``eval_EHF`` keeps the reference's signature and goes through the same call."""
import numpy as np
import torch
from torch.utils.data import Dataset

from .. import _C
from ..body_model.body_model import BodyModel
from ..utils.preprocess import bbox_from_detector, load_ply
from ..utils.transforms import batch_rodrigues, estimate_focal_length

EHF_CAMERA_ROTVEC = (-2.98747896, 0.01172457, -0.05704687)      # mocap_dataset.py:25 (EHF's camera rotation, axis-angle)
EHF_BODY_JOINTS = 22


def regressor_csr(J_regressor, rows=None, device="cuda"):
    """(row_ptr int32 [R + 1], col int32, weight fp32) on ``device``: the non-zeros of the first ``rows`` rows of a joint regressor
    (dense array / tensor or scipy-sparse), columns ascending within a row.  Weights are rounded to fp32 (the kernel's weight type)."""
    if hasattr(J_regressor, "tocsr"):
        m = J_regressor.tocsr()[:rows].astype(np.float32)
        m.sort_indices()
        m.eliminate_zeros()
        ptr, col, w = m.indptr, m.indices, m.data
    else:
        W = (J_regressor.detach().cpu().numpy() if torch.is_tensor(J_regressor) else np.asarray(J_regressor))[:rows].astype(np.float32)
        r, col = np.nonzero(W)                                     # row-major: rows ascending, columns ascending within a row
        ptr = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=W.shape[0]))])
        w = W[r, col]
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a).astype(dt), device=device)
    return t(ptr, np.int32), t(col, np.int32), t(w, np.float32)


def regress_joints(vertices, csr):
    """dposer_regress_joints: joints [B, R, 3] of device meshes ``vertices`` [B, V, 3] under the CSR regressor of ``regressor_csr``."""
    _C.require_gpu(vertices, "regress_joints vertices")
    ptr, col, w = csr
    v = vertices.contiguous().float()
    B, V, R = v.shape[0], v.shape[1], ptr.numel() - 1
    out = torch.empty(B, R, 3, dtype=torch.float32, device=v.device)
    if B:
        args = _C.RegressJointsArgs(v.data_ptr(), B, V, ptr.data_ptr(), col.data_ptr(), w.data_ptr(), R, out.data_ptr())
        _C.check(_C.lib().dposer_regress_joints(args, _C.stream_ptr()), "dposer_regress_joints")
    return out


def ehf_eval(pred_vertices, gt_vertices, csr, gt_rotation=None, pelvis_row=0, return_joints=False):
    """dposer_ehf_eval on device meshes [B, V, 3]: (pa_mpjpe [B], mpjpe [B]) in millimetres, plus (pred_joints, gt_joints,
    aligned_joints) [B, R, 3] with ``return_joints``.  No host synchronisation."""
    _C.require_gpu(pred_vertices, "ehf_eval pred_vertices")
    _C.require_gpu(gt_vertices, "ehf_eval gt_vertices")
    if pred_vertices.dim() != 3 or pred_vertices.shape != gt_vertices.shape or pred_vertices.shape[-1] != 3:
        raise ValueError(f"ehf_eval: meshes must both be [B, V, 3], got {tuple(pred_vertices.shape)} and {tuple(gt_vertices.shape)}")
    ptr, col, w = csr
    pv, gv = pred_vertices.contiguous().float(), gt_vertices.contiguous().float()
    dev = pv.device
    B, V, R = pv.shape[0], pv.shape[1], ptr.numel() - 1
    rot = None if gt_rotation is None else gt_rotation.to(dev).contiguous().float()
    pa, mp = torch.empty(B, dtype=torch.float32, device=dev), torch.empty(B, dtype=torch.float32, device=dev)
    joints = [torch.empty(B, R, 3, dtype=torch.float32, device=dev) for _ in range(3)] if return_joints else [None] * 3
    if B:
        scratch = torch.empty(_C.lib().dposer_ehf_eval_scratch_bytes(B, R), dtype=torch.uint8, device=dev)
        args = _C.EhfEvalArgs(pv.data_ptr(), gv.data_ptr(), B, V, ptr.data_ptr(), col.data_ptr(), w.data_ptr(), R,
                              None if rot is None else rot.data_ptr(), pelvis_row, pa.data_ptr(), mp.data_ptr(),
                              *[None if j is None else j.data_ptr() for j in joints], scratch.data_ptr())
        _C.check(_C.lib().dposer_ehf_eval(args, _C.stream_ptr()), "dposer_ehf_eval")
    return (pa, mp, *joints) if return_joints else (pa, mp)


class MocapDataset(Dataset):
    """mocap_dataset.py:18-88.  ``img_bgr_list`` entries are images [H, W, 3] or bare (h, w) shapes; ``body_model`` (a
    ``body_model.BodyModel``) may be given instead of ``body_model_path``."""

    def __init__(self, img_bgr_list, detection_list, device, body_model_path=None, body_model=None):
        self.img_bgr_list = img_bgr_list
        self.detection_list = detection_list
        self.device = device
        rotvec = torch.tensor([EHF_CAMERA_ROTVEC], dtype=torch.float32, device=device)
        self.cam_param = {"R": batch_rodrigues(rotvec)[0]}         # (the reference: cv2.Rodrigues)
        self.smplx = body_model if body_model is not None else BodyModel(bm_path=body_model_path, num_betas=10, batch_size=1,
                                                                         model_type="smplx").to(device)
        self._csr = regressor_csr(self.smplx.J_regressor, EHF_BODY_JOINTS, device)

    def __len__(self):
        return len(self.detection_list)

    def __getitem__(self, idx):
        """detection row: [image index, min_x, min_y, max_x, max_y]"""
        det = self.detection_list[idx]
        img_idx = int(det[0].item() if hasattr(det[0], "item") else det[0])
        img = self.img_bgr_list[img_idx]
        img_h, img_w = (int(img[0]), int(img[1])) if np.ndim(img) == 1 else img.shape[:2]
        center, scale = bbox_from_detector(det[1:5])
        return {"center": center, "scale": scale, "img_h": img_h, "img_w": img_w, "focal_length": estimate_focal_length(img_h, img_w)}

    def _pred_vertices(self, pred_results):
        pose, betas, camera_translation = pred_results[0], pred_results[1], pred_results[2]
        with torch.no_grad():
            return self.smplx(betas=betas, pose_body=pose[:, 3:66], root_orient=pose[:, :3], trans=camera_translation).v

    def eval_EHF_batch(self, pred_results, gt_vertices):
        """``pred_results`` = (pose [B, 66], betas, camera_translation, ...) as SMPLify returns them, ``gt_vertices`` [B, V, 3] in the
        frame of the EHF scans: {'pa_mpjpe_body': [B], 'mpjpe_body': [B]} as device tensors, without a host synchronisation."""
        gt = torch.as_tensor(gt_vertices, dtype=torch.float32, device=self.device)
        pa, mp = ehf_eval(self._pred_vertices(pred_results), gt, self._csr, self.cam_param["R"], self.smplx.J_regressor_idx["pelvis"])
        return {"pa_mpjpe_body": pa, "mpjpe_body": mp}

    def eval_EHF(self, pred_results, gt_ply_path):
        """mocap_dataset.py:61-84 for the first image of ``pred_results``: {'pa_mpjpe_body': [float], 'mpjpe_body': [float]}."""
        gt = np.asarray(load_ply(gt_ply_path), dtype=np.float32)[None]
        res = self.eval_EHF_batch([p[:1] if torch.is_tensor(p) else p for p in pred_results], gt)
        return {k: [float(v[0])] for k, v in res.items()}

    def print_eval_result(self, eval_result):
        as_np = lambda v: v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)
        print("PA MPJPE (Body): %.2f mm" % np.mean(as_np(eval_result["pa_mpjpe_body"])))
        print("MPJPE (Body): %.2f mm" % np.mean(as_np(eval_result["mpjpe_body"])))
