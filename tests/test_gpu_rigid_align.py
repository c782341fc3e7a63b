"""Batched rigid alignment, joint regression and the EHF evaluation on the GPU (dposer_rigid_align, dposer_regress_joints,
dposer_ehf_eval) and the fitting driver, against the reference's own outputs (golden g29) and the fp64 rule of tests/align_ref.py, which
tests/test_rigid_align_cpu.py pins to g29.

Bounds: aligned points and the action of (c, R, t) within 1e-5 m of the fp64 reference (the project's FK / LBS tolerance); R^T R = I and
det R = 1 to 1e-5 (catches a wrong branch, not rounding); mean distances and both EHF metrics within 1e-2 mm (the same 1e-5 m through a
mean of distances); regressed joints within 1e-6 m (fp64 sums rounded once: half an ulp at 4 m is 2.4e-7).

Measured on an MI355X (DPOSER_LOG_ERR): aligned points <= 9.4e-7 m, action of (c, R, t) <= 5.9e-7 m, R^T R / det R <= 8.5e-8, mean distance
<= 2.0e-4 mm over N = 3 ... 10475; EHF at B = 100: pa_mpjpe 7.3e-5 mm, mpjpe 3.7e-4 mm, joints 9.2e-7 m;
MocapDataset.eval_EHF_batch at B = 100: pa_mpjpe 9.9e-5 mm, mpjpe 2.7e-4 mm."""
import json
import os

import numpy as np
import pytest
import torch

import align_ref
from gpu_common import DEV, t2n
from helpers import _log_measured, load

pytestmark = pytest.mark.gpu

TOL_M = 1e-5
TOL_MM = 1e-2
TOL_ROT = 1e-5
TOL_JOINT = 1e-6


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=DEV)


def _align(src, dst, **kw):
    from dposer_amd.utils.transforms import rigid_align_device
    return rigid_align_device(_dev(src), _dev(dst), **kw)


def _check_against_reference(src, dst, tag):
    """One call over the batch; every pair against align_ref.  Returns the measured maxima."""
    T, aligned, md = _align(src, dst)
    T, aligned, md = t2n(T).astype(np.float64), t2n(aligned), t2n(md)
    e_al = e_act = e_rot = e_md = 0.0
    for k in range(len(src)):
        ref = align_ref.align(src[k], dst[k])
        c, R, t = T[k, 0], T[k, 1:10].reshape(3, 3), T[k, 10:]
        e_al = max(e_al, np.abs(aligned[k] - ref).max())
        e_act = max(e_act, np.abs(c * (src[k].astype(np.float64) @ R.T) + t - ref).max())
        e_rot = max(e_rot, np.abs(R.T @ R - np.eye(3)).max(), abs(np.linalg.det(R) - 1.0))
        e_md = max(e_md, abs(float(md[k]) - align_ref.mean_distance(ref, dst[k])) * 1000)
    for kind, v in (("aligned_m", e_al), ("action_m", e_act), ("rotation", e_rot), ("mean_dist_mm", e_md)):
        _log_measured(f"{tag}_{kind}", v)
    print(f"{tag}: aligned {e_al:.2e} m, action {e_act:.2e} m, rotation {e_rot:.2e}, mean_dist {e_md:.2e} mm")
    assert e_al <= TOL_M and e_act <= TOL_M and e_rot <= TOL_ROT and e_md <= TOL_MM, (tag, e_al, e_act, e_rot, e_md)
    return e_al, e_act, e_rot, e_md


# ---- 1. hand cases
def test_hand_cases_match_the_reference_golden():
    g = load("g29_rigid_align")
    for nm in g["hand_names"]:
        A, B = g[f"hand_{nm}_src"], g[f"hand_{nm}_dst"]
        T, aligned, md = _align(A[None], B[None])
        T = t2n(T)[0].astype(np.float64)
        R = T[1:10].reshape(3, 3)
        e = np.abs(t2n(aligned)[0] - g[f"hand_{nm}_aligned"]).max()
        _log_measured(f"hand_{nm}_aligned_m", e)
        assert e <= TOL_M, (nm, e)
        assert abs(np.linalg.det(R) - 1) <= TOL_ROT and np.abs(R.T @ R - np.eye(3)).max() <= TOL_ROT, nm     # a proper rotation, mirrored included
        assert np.abs(R - g[f"hand_{nm}_R"]).max() <= 1e-5 and abs(T[0] - g[f"hand_{nm}_c"]) <= 1e-5 * g[f"hand_{nm}_c"], nm
        assert abs(float(md[0]) - align_ref.mean_distance(g[f"hand_{nm}_aligned"], B)) * 1000 <= TOL_MM
    # identity and a known similarity, recovered
    T = t2n(_align(g["hand_identity_src"][None], g["hand_identity_dst"][None])[0])[0]
    assert np.abs(T - np.array([1, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32)).max() <= 1e-6
    from scipy.spatial.transform import Rotation
    T = t2n(_align(g["hand_similarity_src"][None], g["hand_similarity_dst"][None])[0])[0]
    assert abs(T[0] - 1.3) <= 1e-5 and np.abs(T[1:10].reshape(3, 3) - Rotation.from_rotvec([0.3, -1.1, 0.6]).as_matrix()).max() <= 1e-5
    assert np.abs(T[10:] - [0.5, 2.0, -1.0]).max() <= 1e-5


def test_degenerate_pairs_are_non_finite_and_leave_their_neighbours_alone():
    src, dst = align_ref.kept_pairs(22, 8, 4100)
    src, dst = src.copy(), dst.copy()
    ref = _align(src, dst)
    src[2] = src[2, 0]                                       # zero variance
    src[5, 7, 1] = np.nan
    dst[6, 0, 0] = np.inf
    T, aligned, md = _align(src, dst)
    for k in range(8):
        bad = k in (2, 5, 6)
        for got, want in zip((T, aligned, md), ref):
            if bad:
                assert not torch.isfinite(got[k]).any(), k
            else:
                assert torch.equal(got[k], want[k]), k
    # N = 1: the variance of one point is zero
    T, aligned, md = _align(src[:3, :1], dst[:3, :1])
    assert not torch.isfinite(T).any() and not torch.isfinite(aligned).any() and not torch.isfinite(md).any()


# ---- 2. golden and generated sets
@pytest.mark.parametrize("n", [4, 22, 55])
def test_golden_sets(n):
    g = load("g29_rigid_align")
    kept = g[f"ra{n}_kept"]
    src, dst = g[f"ra{n}_src"][kept], g[f"ra{n}_dst"][kept]
    _check_against_reference(src, dst, f"g29_n{n}")
    T, aligned, _ = _align(src, dst)
    e = np.abs(t2n(aligned) - g[f"ra{n}_aligned"][kept]).max()
    _log_measured(f"g29_n{n}_vs_reference_m", e)
    assert e <= TOL_M
    assert (np.linalg.det(t2n(T)[:, 1:10].reshape(-1, 3, 3).astype(np.float64)) > 0).all()


@pytest.mark.parametrize("n,count", [(4, 200), (22, 200), (55, 200), (64, 100), (65, 100), (10475, 10)])
def test_generated_sets(n, count):
    src, dst = align_ref.kept_pairs(n, count, 1000 + n)
    _check_against_reference(src, dst, f"gen_n{n}")


def test_triangles():
    """N = 3 by hand-built triangles (the generator's gate would drop 8 % of random ones)."""
    g = load("g29_rigid_align")
    src = np.stack([g["hand_triangle_src"], g["hand_triangle2_src"]])
    dst = np.stack([g["hand_triangle_dst"], g["hand_triangle2_dst"]])
    _check_against_reference(src, dst, "triangles")


# ---- 3. bit identity
@pytest.mark.parametrize("n", [22, 64, 65, 300])
def test_bits_do_not_depend_on_the_batch(n):
    src, dst = align_ref.kept_pairs(n, 24, 5000 + n)
    full = _align(src, dst)
    B = len(src)
    for k in range(B):                                       # each pair alone
        one = _align(src[k:k + 1], dst[k:k + 1])
        assert all(torch.equal(a[0], b[k]) for a, b in zip(one, full)), k
    bounds = [0, 1, 4, 9, 10, 17, B]                         # uneven groups
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        part = _align(src[lo:hi], dst[lo:hi])
        assert all(torch.equal(a, b[lo:hi]) for a, b in zip(part, full)), (lo, hi)
    rev = _align(src[::-1], dst[::-1])
    assert all(torch.equal(a.flip(0), b) for a, b in zip(rev, full))
    # NULL optional outputs change nothing else
    for kw in (dict(aligned=False), dict(transform=False), dict(mean_dist=False), dict(transform=False, aligned=False),
               dict(aligned=False, mean_dist=False)):
        part = _align(src, dst, **kw)
        for a, b in zip(part, full):
            assert a is None or torch.equal(a, b), kw


# ---- 4. joint regression
def _asset():
    from dposer_amd.body_model.synthetic import make_synthetic_smplx_asset
    return make_synthetic_smplx_asset(seed=0)


def _bodies(B, seed, asset=None):
    """Predicted meshes of B random bodies metres from the origin and ground-truth meshes of other bodies under a similarity, fp32 device."""
    from dposer_amd.body_model.body_model import BodyModel
    bm = BodyModel(asset or _asset()).to(DEV)
    gen = torch.Generator(device=DEV).manual_seed(seed)
    r = lambda *s: torch.randn(*s, device=DEV, generator=gen)
    with torch.no_grad():
        pred = bm(pose_body=r(B, 63) * 0.3, root_orient=r(B, 3) * 0.5, betas=r(B, 10) * 0.5, trans=r(B, 3) * 2 + torch.tensor([0.0, 0, 3], device=DEV)).v
        gt = bm(pose_body=r(B, 63) * 0.3, root_orient=r(B, 3) * 0.5, betas=r(B, 10) * 0.5).v
    from scipy.spatial.transform import Rotation
    rs = np.random.RandomState(seed)
    Rk = _dev(Rotation.from_rotvec(rs.standard_normal((B, 3))).as_matrix())
    gt = torch.einsum("bvk,bjk->bvj", gt, Rk) * _dev(rs.uniform(0.8, 1.25, (B, 1, 1))) + _dev(rs.uniform(-3, 3, (B, 1, 3)))
    return bm, pred.contiguous(), gt.contiguous()


@pytest.mark.parametrize("sparse", [False, True])
def test_regress_joints(sparse):
    import scipy.sparse
    from dposer_amd.dataset.mocap_dataset import regress_joints, regressor_csr
    asset = _asset()
    J = asset["J_regressor"]
    csr = regressor_csr(scipy.sparse.csc_matrix(J) if sparse else J, 22, DEV)
    assert csr[0].numel() == 23 and int(csr[0][-1]) == int((J[:22] != 0).sum())
    _, pred, _ = _bodies(16, 41, asset)
    out = t2n(regress_joints(pred, csr))
    ref = align_ref.regress(J, t2n(pred))
    e = np.abs(out - ref).max()
    _log_measured("regress_joints_m", e)
    assert np.abs(ref).max() > 3.0 and e <= TOL_JOINT, e
    full = t2n(regress_joints(pred, regressor_csr(J, None, DEV)))         # every row
    assert full.shape == (16, 55, 3) and np.array_equal(full[:, :22], out)


# ---- 5. the EHF evaluation
def _mocap(asset=None):
    from dposer_amd.body_model.body_model import BodyModel
    from dposer_amd.dataset.mocap_dataset import MocapDataset
    bm = BodyModel(asset or _asset()).to(DEV)
    return MocapDataset([(1200, 1600)], np.array([[0, 400, 100, 1000, 1200]]), DEV, body_model=bm)


def test_ehf_rotation_is_the_rodrigues_matrix_of_the_reference_vector():
    g = load("g29_rigid_align")
    R = t2n(_mocap().cam_param["R"])
    assert np.abs(R - g["ehf_rotation"]).max() <= 1e-6


def test_ehf_eval_at_ehf_size():
    from dposer_amd.dataset.mocap_dataset import ehf_eval, regressor_csr
    asset = _asset()
    J = asset["J_regressor"]
    B = 100
    _, pred, gt = _bodies(B, 43, asset)
    db = _mocap(asset)
    R = db.cam_param["R"]
    pa, mp, jp, jg, ja = ehf_eval(pred, gt, regressor_csr(J, 22, DEV), R, 0, return_joints=True)
    pa2, mp2 = ehf_eval(pred, gt, regressor_csr(J, 22, DEV), R, 0)
    assert torch.equal(pa, pa2) and torch.equal(mp, mp2)
    pn, gn, Rn = t2n(pred), t2n(gt), t2n(R).astype(np.float64)
    e_pa = e_mp = e_j = 0.0
    for k in range(B):
        rpa, rmp = align_ref.ehf_metrics(J, pn[k], gn[k], Rn)
        e_pa, e_mp = max(e_pa, abs(float(pa[k]) - rpa)), max(e_mp, abs(float(mp[k]) - rmp))
        rj = align_ref.regress(J, gn[k]) @ Rn.T
        e_j = max(e_j, np.abs(t2n(jg[k]) - rj).max(), np.abs(t2n(jp[k]) - align_ref.regress(J, pn[k])).max(),
                  np.abs(t2n(ja[k]) - align_ref.align(align_ref.regress(J, pn[k]), rj)).max())
    for kind, v in (("ehf_pa_mpjpe_mm", e_pa), ("ehf_mpjpe_mm", e_mp), ("ehf_joints_m", e_j)):
        _log_measured(kind, v)
    print(f"ehf_eval B = 100: pa_mpjpe {e_pa:.2e} mm, mpjpe {e_mp:.2e} mm, joints {e_j:.2e} m")
    assert e_pa <= TOL_MM and e_mp <= TOL_MM and e_j <= TOL_M, (e_pa, e_mp, e_j)
    assert float(pa.min()) > 1.0 and float(mp.max()) > 100.0           # (different bodies: the metrics are not trivially zero)
    # independent of the batch
    for k in (0, 57, 99):
        a, b = ehf_eval(pred[k:k + 1], gt[k:k + 1], regressor_csr(J, 22, DEV), R, 0)
        assert torch.equal(a[0], pa[k]) and torch.equal(b[0], mp[k])


def test_ehf_eval_matches_the_reference_record():
    from dposer_amd.dataset.mocap_dataset import ehf_eval, regressor_csr
    g = load("g29_rigid_align")
    J = _asset()["J_regressor"]
    used = g["ehf_used_vertices"]
    n = len(g["ehf_pa_mpjpe"])
    pred, gt = np.zeros((n, J.shape[1], 3), np.float32), np.zeros((n, J.shape[1], 3), np.float32)
    pred[:, used], gt[:, used] = g["ehf_pred_used"], g["ehf_gt_used"]
    pa, mp = ehf_eval(_dev(pred), _dev(gt), regressor_csr(J, 22, DEV), _mocap().cam_param["R"], 0)
    e_pa, e_mp = np.abs(t2n(pa) - g["ehf_pa_mpjpe"]).max(), np.abs(t2n(mp) - g["ehf_mpjpe"]).max()
    _log_measured("g29_ehf_pa_mpjpe_mm", e_pa)
    _log_measured("g29_ehf_mpjpe_mm", e_mp)
    assert e_pa <= TOL_MM and e_mp <= TOL_MM, (e_pa, e_mp)


def _pred_results(B, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    r = lambda *s: torch.randn(*s, device=DEV, generator=gen)
    pose = torch.cat([r(B, 3) * 0.5, r(B, 63) * 0.3], 1)
    return pose, r(B, 10) * 0.5, r(B, 3) + torch.tensor([0.0, 0, 4], device=DEV), None


def test_eval_ehf_batch_at_ehf_size_against_the_fp64_rule():
    """MocapDataset.eval_EHF_batch itself at B = 100: its mapping of (pose, betas, camera translation) onto the body model, its camera
    rotation, pelvis row and 22-row regressor, against align_ref on meshes the test forms by hand and the rotation matrix of the reference
    record (g29, scipy's), within the 1e-2 mm bound."""
    g = load("g29_rigid_align")
    asset = _asset()
    J = asset["J_regressor"]
    db = _mocap(asset)
    B = 100
    res = _pred_results(B, 53)
    pose, betas, cam_t, _ = res
    _, _, gt = _bodies(B, 54, asset)
    out = db.eval_EHF_batch(res, gt)
    assert out["pa_mpjpe_body"].is_cuda and out["pa_mpjpe_body"].shape == (B,) and out["mpjpe_body"].shape == (B,)
    with torch.no_grad():
        verts = t2n(db.smplx(root_orient=pose[:, :3].contiguous(), pose_body=pose[:, 3:66].contiguous(), betas=betas, trans=cam_t).v)
    gn = t2n(gt)
    e_pa = e_mp = 0.0
    for k in range(B):
        rpa, rmp = align_ref.ehf_metrics(J, verts[k], gn[k], g["ehf_rotation"], pelvis=0, rows=22)
        e_pa = max(e_pa, abs(float(out["pa_mpjpe_body"][k]) - rpa))
        e_mp = max(e_mp, abs(float(out["mpjpe_body"][k]) - rmp))
    _log_measured("eval_ehf_batch_pa_mpjpe_mm", e_pa)
    _log_measured("eval_ehf_batch_mpjpe_mm", e_mp)
    print(f"eval_EHF_batch B = 100: pa_mpjpe {e_pa:.2e} mm, mpjpe {e_mp:.2e} mm")
    assert e_pa <= TOL_MM and e_mp <= TOL_MM, (e_pa, e_mp)
    # the rotation matters (its transpose, or none, moves MPJPE by far more than the bound): the check above can tell them apart
    wrong = align_ref.ehf_metrics(J, verts[0], gn[0], g["ehf_rotation"].T)[1]
    assert abs(wrong - float(out["mpjpe_body"][0])) > 1.0


def test_eval_ehf_from_a_ply_file_equals_the_batch_entry(tmp_path):
    db = _mocap()
    B = 5
    res = _pred_results(B, 47)
    _, _, gt = _bodies(B, 48)
    batch = db.eval_EHF_batch(res, gt)
    assert batch["pa_mpjpe_body"].is_cuda and batch["pa_mpjpe_body"].shape == (B,)
    for k, fmt in ((0, "binary_little_endian"), (3, "ascii"), (4, "binary_big_endian")):
        p = str(tmp_path / f"gt{k}.ply")
        align_ref.write_ply(p, t2n(gt[k]), fmt, faces=[[0, 1, 2]])
        one = db.eval_EHF([x[k:k + 1] if x is not None else None for x in res], p)
        assert set(one) == {"pa_mpjpe_body", "mpjpe_body"} and isinstance(one["pa_mpjpe_body"], list)
        assert one["pa_mpjpe_body"][0] == float(batch["pa_mpjpe_body"][k]) and one["mpjpe_body"][0] == float(batch["mpjpe_body"][k])


# ---- 6. the host functions
def test_rigid_align_host_functions():
    from dposer_amd.utils.transforms import rigid_align, rigid_transform_3D
    src, dst = align_ref.kept_pairs(22, 8, 6100)
    T, aligned, _ = _align(src, dst)
    out = rigid_align(src, dst)                                  # numpy in -> numpy out, [B, N, 3]
    assert isinstance(out, np.ndarray) and out.dtype == np.float32 and np.array_equal(out, t2n(aligned))
    one = rigid_align(src[2].astype(np.float64), dst[2].astype(np.float64))      # [N, 3], fp64 as eval_EHF hands it over
    assert one.dtype == np.float64 and one.shape == (22, 3) and np.array_equal(one, t2n(aligned[2]).astype(np.float64))
    c, R, t = rigid_transform_3D(src[1], dst[1])
    assert R.shape == (3, 3) and t.shape == (3,) and np.ndim(c) == 0
    assert np.array_equal(np.concatenate([[c], R.reshape(-1), t]), t2n(T[1]))
    dc, dR, dt = rigid_transform_3D(_dev(src), _dev(dst))         # device in -> device out
    assert dc.is_cuda and dR.shape == (8, 3, 3) and torch.equal(torch.cat([dc[:, None], dR.reshape(8, 9), dt], 1), T)
    assert torch.equal(rigid_align(_dev(src), _dev(dst)), aligned) and torch.equal(rigid_align(_dev(src[0]), _dev(dst[0])), aligned[0])
    with pytest.raises(ValueError):
        rigid_align(src[:, :, :2], dst[:, :, :2])


# ---- 7. addressing past 2^31 elements
def test_one_call_past_two_billion_coordinates():
    """68400 pairs x 10475 points x 3 = 2.15e9 coordinates per input (8.6 GB each), aligned NULL: the first and the last pairs come out as
    the fp64 reference's and as the same pairs by themselves."""
    from dposer_amd.utils.transforms import rigid_align_device
    B, N = 68400, 10475
    gen = torch.Generator(device=DEV).manual_seed(7)
    src = torch.randn(B, N, 3, device=DEV, generator=gen)
    src.mul_(torch.tensor([0.4, 0.25, 0.1], device=DEV)).add_(torch.tensor([1.0, -2.0, 3.0], device=DEV))
    assert src.numel() > 2 ** 31
    dst = torch.randn(B, N, 3, device=DEV, generator=gen).mul_(0.03)
    dst.add_(src.flip(2) * 1.2)                                 # a reflected similarity (axes swapped) plus noise
    T, _, md = rigid_align_device(src, dst, aligned=False)
    for k in (0, 1, B // 2, B - 2, B - 1):
        a, b = t2n(src[k]), t2n(dst[k])
        c, R, t = align_ref.similarity(a, b)
        Tk = t2n(T[k]).astype(np.float64)
        act = Tk[0] * (a.astype(np.float64) @ Tk[1:10].reshape(3, 3).T) + Tk[10:]
        ref = align_ref.align(a, b)
        assert np.abs(act - ref).max() <= TOL_M and abs(float(md[k]) - align_ref.mean_distance(ref, b)) * 1000 <= TOL_MM, k
        T1, _, md1 = rigid_align_device(src[k:k + 1], dst[k:k + 1], aligned=False)
        assert torch.equal(T1[0], T[k]) and torch.equal(md1[0], md[k]), k
    assert torch.isfinite(T).all() and torch.isfinite(md).all()
    del src, dst, T, md
    torch.cuda.empty_cache()


# ---- 8. the driver
def _driver_case(tmp_path, B):
    """A folder like EHF's: photos (uint8 arrays), OpenPose JSON keypoints projected from known bodies, .ply ground truth."""
    from test_gpu_smplify import _smplify
    from dposer_amd.utils.transforms import estimate_focal_length
    sm = _smplify(B, 2)
    db = _mocap()
    rs = np.random.RandomState(80)
    shapes = [(120, 160), (96, 128), (120, 160)][:B]
    boxes = np.array([[0, 40, 10, 100, 110], [0, 30, 8, 90, 90], [0, 50, 12, 120, 112]], np.float64)[:B]
    images = [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in shapes]
    _, _, gt = _bodies(B, 81)
    kps = []
    for k, (h, w) in enumerate(shapes):
        f = estimate_focal_length(h, w)
        with torch.no_grad():
            j = sm.smpl(betas=torch.zeros(1, 10, device=DEV), body_pose=torch.zeros(1, 63, device=DEV) + 0.05 * k,
                        global_orient=torch.tensor([[3.0, 0.1, 0.0]], device=DEV), transl=torch.tensor([[0.0, 0.1, 3.5]], device=DEV)).joints[0, :25]
        j = t2n(j).astype(np.float64)
        kp = np.concatenate([f * j[:, :2] / j[:, 2:] + [w / 2, h / 2], rs.uniform(0.3, 1.0, (25, 1))], 1)
        kps.append(kp)
        with open(tmp_path / f"{k:02d}_2Djnt.json", "w") as fh:
            json.dump({"people": [{"pose_keypoints_2d": kp.reshape(-1).tolist()}]}, fh)
        align_ref.write_ply(str(tmp_path / f"{k:02d}_align.ply"), t2n(gt[k]))
    return sm, db, np.stack(kps), shapes, boxes, images, gt


def test_fit_and_evaluate_is_the_pipeline_by_hand(tmp_path):
    from dposer_amd.tasks.fitting import fit_and_evaluate, initial_fit
    B = 3
    sm, db, kps, shapes, boxes, images, gt = _driver_case(tmp_path, B)
    calls = sm.pose_prior._calls                               # (the prior's noise counter: the same start for both runs)
    out = fit_and_evaluate(sm, db, kps, shapes, gt, boxes, images=images, outdir=str(tmp_path / "out"), seed=5)
    sm.pose_prior._calls = calls
    init = initial_fit(sm.smpl, kps, shapes, boxes)
    sm.focal_length = init["focal_length"]
    res = sm(init["init_pose"], init["init_betas"], init["init_cam_t"], init["camera_center"], init["keypoints"], seed=5)
    for a, b in zip(res, (out["pose"], out["betas"], out["camera_translation"], out["reprojection_loss"])):
        assert torch.equal(a, b)
    ev = db.eval_EHF_batch(res, gt)
    assert torch.equal(ev["pa_mpjpe_body"], out["pa_mpjpe_body"]) and torch.equal(ev["mpjpe_body"], out["mpjpe_body"])
    assert torch.isfinite(out["pa_mpjpe_body"]).all() and out["vertices"].shape == (B, 10475, 3)
    with torch.no_grad():                                      # the body model by hand
        verts = sm.smpl(betas=res[1], body_pose=res[0][:, 3:], global_orient=res[0][:, :3], pose2rot=True, transl=res[2]).vertices
    assert torch.equal(verts, out["vertices"])
    # every overlay is what the existing Renderer.render_front_view gives for that image alone
    from dposer_amd.body_model.visual import Renderer
    for k in range(B):
        h, w = shapes[k]
        rd = Renderer(focal_length=init["focal_length"][k], img_w=w, img_h=h, faces=sm.smpl.faces, same_mesh_color=True)
        front = rd.render_front_view(verts[k:k + 1], bg_img_rgb=images[k].copy())
        assert np.array_equal(front, t2n(out["overlays"][k])), k
    # the overlay differs from the photo exactly where the depth output is positive
    for k in range(B):
        ov, depth = t2n(out["overlays"][k]), t2n(out["depth"][k])
        assert ov.shape == images[k].shape and depth.shape == shapes[k]
        assert np.array_equal((ov != images[k]).any(-1), depth > 0) and (depth > 0).sum() > 20, k
        assert os.path.getsize(tmp_path / "out" / f"{k:06d}_mesh_fit.png") > 100


def test_reference_shaped_path_agrees_with_the_batched_path(tmp_path):
    """run/fitting.py's own sequence for one image -- MocapDataset + DataLoader + cam_crop2full + SMPLify + eval_EHF on the .ply -- against
    fit_and_evaluate on the same image."""
    from torch.utils.data import DataLoader
    from dposer_amd.dataset.mocap_dataset import MocapDataset
    from dposer_amd.tasks.fitting import fit_and_evaluate
    from dposer_amd.utils.transforms import cam_crop2full
    sm, db, kps, shapes, boxes, images, gt = _driver_case(tmp_path, 1)
    calls = sm.pose_prior._calls                               # (the prior's noise counter: the same start for both runs)
    out = fit_and_evaluate(sm, db, kps, shapes, gt, boxes, seed=5)
    sm.pose_prior._calls = calls
    mocap_db = MocapDataset([images[0][:, :, ::-1]], boxes, device=DEV, body_model=db.smplx)
    for batch in DataLoader(mocap_db, batch_size=1, num_workers=0):
        center, scale = batch["center"].to(DEV).float(), batch["scale"].to(DEV).float()
        img_h, img_w = batch["img_h"].to(DEV).float(), batch["img_w"].to(DEV).float()
        focal_length = batch["focal_length"].to(DEV).float()
        kpts = np.zeros((1, 49, 3))
        kpts[0, :25, :] = kps[0]
        full_img_shape = torch.stack((img_h, img_w), dim=-1)
        init_cam_t = cam_crop2full(torch.tensor([[0.9, 0, 0]], device=DEV), center, scale, full_img_shape, focal_length)
        smpl_poses = sm.smpl.mean_poses[:66].unsqueeze(0)
        init_betas = sm.smpl.mean_shape.unsqueeze(0)
        camera_center = torch.hstack((img_w[:, None], img_h[:, None])) / 2
        sm.focal_length = focal_length
        results = sm(smpl_poses, init_betas, init_cam_t, camera_center, torch.from_numpy(kpts).to(DEV), seed=5)
        ev = mocap_db.eval_EHF(results, str(tmp_path / "00_align.ply"))
    assert torch.equal(init_cam_t, out["init"]["init_cam_t"]) and torch.equal(focal_length, out["init"]["focal_length"])
    assert torch.equal(results[0], out["pose"]) and torch.equal(results[2], out["camera_translation"])
    assert ev["pa_mpjpe_body"][0] == float(out["pa_mpjpe_body"][0]) and ev["mpjpe_body"][0] == float(out["mpjpe_body"][0])


def test_run_folder(tmp_path, capsys):
    from dposer_amd.tasks.fitting import fit_and_evaluate, run_folder
    sm, db, kps, shapes, boxes, images, gt = _driver_case(tmp_path, 3)
    calls = sm.pose_prior._calls                               # (the prior's noise counter: the same start for both runs)
    res = run_folder(str(tmp_path), str(tmp_path / "out"), sm, db, batch_size=2, image_shapes=shapes, fixed_box=None, bend_min_y=1e9, seed=5)
    sm.pose_prior._calls = calls
    assert "PA MPJPE (Body):" in capsys.readouterr().out and len(res["pa_mpjpe_body"]) == 3
    kbox = np.stack([[0, k[:, 0].min(), k[:, 1].min(), k[:, 0].max(), k[:, 1].max()] for k in kps])
    first = fit_and_evaluate(sm, db, kps[:2], shapes[:2], gt[:2], kbox[:2], seed=5)
    assert res["pa_mpjpe_body"][:2] == first["pa_mpjpe_body"].cpu().tolist()
