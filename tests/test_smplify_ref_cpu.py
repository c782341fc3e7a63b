"""The float64 SMPLify loop of oracle/task_loops.py is checked here before it judges the kernels (tests/test_gpu_smplify.py): against the
reference's own loop and loss captures (golden g27), for the distance of its float32 run from its float64 run over the GPU case matrix
(the band the GPU tolerance is 8 x of), and for sharpness -- nine seeded faults each leave that tolerance by more than 10 x."""
import numpy as np
import pytest
import torch

import smplify_cases as SC
from helpers import load
from oracle import fk_torch
from oracle import score_ref as R
from oracle import task_loops as TL


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def test_vertex_subset_keeps_every_mapped_joint():
    """The oracle loop skins only the vertices a mapped joint reads; the 49 joints of that asset are those of the whole mesh."""
    full, sub = SC.assets()
    jmap, _ = SC.joint_tables()
    assert sub["v_template"].shape[0] < full["v_template"].shape[0] // 4
    rs = np.random.RandomState(1)
    d = lambda *s, k: torch.tensor(rs.standard_normal(s) * k)
    bp, bt, go, tr = d(3, 63, k=0.3), d(3, 10, k=0.5), d(3, 3, k=0.3), d(3, 3, k=1.0)
    ja = fk_torch.smplx_forward(full, bp, betas=bt, global_orient=go, transl=tr)[1][:, jmap]
    jb = fk_torch.smplx_forward(sub, bp, betas=bt, global_orient=go, transl=tr)[1][:, jmap]
    assert (ja - jb).abs().max().item() < 1e-13


def _g27_run(dtype):
    g = load("g27_smplify")
    g10 = load("g10_normalizer")
    jmap, tab = SC.joint_tables()
    p = SC.params("axis")
    assert int(g["seed"]) == SC.SEED and int(g["sde_N"]) == SC.SDE_N and int(g["num_iters"]) == SC.NUM_ITERS
    ts = torch.linspace(1.0, 1e-3, SC.SDE_N)
    t_list = [float(ts[q]) for q in g["quan_t"]]
    assert t_list == SC.t_list()                      # the cases' schedule is the one the reference drew
    return TL.smplify_optimize(p, R.SubVP(N=SC.SDE_N), SC.assets()[1], jmap, g["init_pose"], g["init_betas"], g["init_cam_t"], g["camera_center"],
                               g["keypoints"], t_list, g["noise"], focal_length=g["focal_length"], num_iters=SC.NUM_ITERS, norm_mode="zscore",
                               norm_a=g10["stats/axis_normalize2/mean_poses"], norm_b=g10["stats/axis_normalize2/std_poses"], dtype=dtype, **tab)


def test_oracle_matches_the_reference_loop():
    """Golden g27 is the reference's own SMPLify.__call__ with an fp64 body-model stand-in and fp32 everything else: a second sample of
    the rounding noise that separates the oracle's float32 run from its float64 run.  So the float64 oracle is held to g27 within 4 x
    that distance, quantity by quantity (measured: 0.5 x to 1.0 x; finals ~2e-7, reprojection 1.1e-6), on the outputs AND on the
    parameters the reference's body model saw at every one of its 19 calls."""
    g = load("g27_smplify")
    a, b = _g27_run(torch.float64), _g27_run(torch.float32)
    for k, gk in (("pose", "pose"), ("betas", "betas"), ("cam_t", "cam_t"), ("reprojection", "reprojection_loss"), ("it_orient", "it_orient"),
                  ("it_body_pose", "it_body_pose"), ("it_betas", "it_betas"), ("it_transl", "it_transl")):
        assert a[k].shape == g[gk].shape
        d_ref, d32 = _rel(a[k], g[gk]), _rel(b[k], a[k])
        print(f"g27 {k}: float64 vs reference {d_ref:.2e}, float32 vs float64 {d32:.2e}")
        assert d32 < 1e-5 and d_ref <= 4 * d32, (k, d_ref, d32)
    assert np.array_equal(a["conf"].astype(np.float32), g["keypoints_after"][:, :, 2])
    # the per-image prior shares add up to the logged batch term
    assert np.allclose(a["prior_terms"].sum(axis=1), a["log"][SC.NUM_ITERS:, 0, 3], rtol=1e-12)


def test_oracle_loss_terms_match_the_reference_captures():
    """The oracle's loss terms at the recorded ``lc_*`` inputs against the reference's fitting_losses values and autograd gradients (fp32
    records: 1e-5 relative on the values the reference sums over ~400 terms, 1e-5 of the largest entry on the gradients)."""
    g = load("g27_smplify")
    _, tab = SC.joint_tables()
    d = lambda k: torch.tensor(np.asarray(g[k], np.float64))
    kp, focal, center = d("keypoints"), d("focal_length"), d("camera_center")

    def close(got, want):
        want = np.asarray(want, np.float64)
        assert np.abs(got.numpy() - want).max() <= 1e-5 * np.abs(want).max(), float(np.abs(got.numpy() - want).max())

    for tag in ("none", "const"):
        jv, bp, bt = (d(k).requires_grad_(True) for k in ("lc_joints", "lc_body_pose", "lc_betas"))
        rep, ang, shp = TL.smplify_body_terms(bp, bt, jv, center, kp[:, :, :2], kp[:, :, 2], focal)      # the defaults of fitting_losses.py:61-62
        prior = 4.78 ** 2 * (bp ** 2).sum() / bp.shape[0] if tag == "const" else 0.0
        loss = (rep.sum(dim=-1) + ang + shp + prior).mean()
        loss.backward()
        assert abs(loss.item() - float(g[f"lc_body_{tag}_loss"])) <= 1e-5 * abs(float(g[f"lc_body_{tag}_loss"]))
        close(jv.grad, g[f"lc_body_{tag}_djoints"])
        close(bp.grad, g[f"lc_body_{tag}_dbody_pose"])
        close(bt.grad, g[f"lc_body_{tag}_dbetas"])
        close(rep.detach(), g[f"lc_body_{tag}_reproj"])
    jv, ct = d("lc_joints").requires_grad_(True), d("lc_cam_t").requires_grad_(True)
    rep, depth = TL.smplify_camera_terms(jv, ct, d("lc_cam_est"), center, kp[:, :, :2], kp[:, :, 2], focal, tab["op_joints"], tab["gt_joints"])
    loss = (rep + depth).sum()
    loss.backward()
    assert abs(loss.item() - float(g["lc_cam_loss"])) <= 1e-5 * abs(float(g["lc_cam_loss"]))
    close(jv.grad, g["lc_cam_djoints"])
    close(ct.grad, g["lc_cam_dcam_t"])
    # image 1 of g27 has no OP RHip detection: the four GT joints carry its gradient, and no OP joint does
    assert (jv.grad[1, tab["op_joints"]] == 0).all() and (jv.grad[1, tab["gt_joints"]] != 0).any()
    assert (jv.grad[0, tab["gt_joints"]] == 0).all()


def test_float32_oracle_stays_inside_the_band():
    """Every case of the GPU matrix in float32 against float64.  The maxima are the D32 constants the GPU tolerance is 8 x of: every
    case must sit inside that tolerance (torch-fp32 itself passes the test the kernels take), and the committed constants must still be
    the measured maxima -- within 3 x either way, the scatter of one rounding sample on another host's BLAS."""
    worst = {k: 0.0 for k in SC.D32}
    for name in SC.CASES:
        d = SC.distances(SC.run_oracle(name, torch.float32), SC.reference(name))
        print(name, " ".join(f"{k}={v:.2e}" for k, v in d.items()))
        for k, v in d.items():
            assert v < SC.TOL[k], (name, k, v, SC.TOL[k])
            worst[k] = max(worst[k], v)
        ref = SC.reference(name)
        assert (ref["log"][:SC.NUM_ITERS, :, 1:3] == 0).all() and np.isfinite(ref["log"]).all()
    print("d32 maxima:", " ".join(f"{k}={v:.2e}" for k, v in worst.items()))
    for k, v in worst.items():
        assert SC.D32[k] / 3 <= v <= SC.D32[k] * 3, (k, v, SC.D32[k])


def test_the_edge_cases_are_the_edges_they_claim():
    _, tab = SC.joint_tables()
    x, ref = SC.inputs("conf_edges"), SC.reference("conf_edges")
    assert (x["keypoints"][0, :, 2] == 0).all() and x["keypoints"][3, tab["op_joints"][3], 2] == -0.5
    # the image without a confident keypoint: no reprojection term in its body stage, and a zero final reprojection
    assert (ref["log"][SC.NUM_ITERS:, 0, 0] == 0).all() and (ref["reprojection"][0] == 0).all() and (ref["log"][SC.NUM_ITERS:, 1:, 0] > 0).all()
    # the negative confidence survives the zeroing (it is no ignored joint) and weighs 0.25 in the final reprojection
    assert ref["conf"][3, tab["op_joints"][3]] == -0.5 and ref["reprojection"][3, tab["op_joints"][3]] > 0
    assert (SC.inputs("zero_pose_axis")["init_pose"][:, 3:] == 0).all() and (SC.inputs("zero_pose_rot6d")["init_pose"][:, 3:] == 0).all()
    assert isinstance(SC.inputs("b1_scalar_focal")["focal_length"], float) and SC.inputs("b1_scalar_focal")["init_pose"].shape[0] == 1
    for name in SC.CASES:
        assert all(np.isfinite(v).all() for v in SC.inputs(name).values())


# fault -> the cases it is seeded into (measured: the largest distance / tolerance over the compared quantities)
FAULT_CASES = {
    "gt_fallback_ignored": ("axis_zscore", "conf_edges"),            # 2.1e4 (camera log column 0), 4.1e4
    "ign_joint_kept": ("axis_zscore",),                              # 3.4e3 (reprojection)
    "gmof_plain_square": ("axis_zscore",),                           # 4.4e4 (body log column 0)
    "min_max_without_2": ("axis_minmax", "rot6d_minmax"),            # 3.2e3 (pose), 3.3e3 (reprojection)
    "angle_sign_55": ("axis_zscore",),                               # 4.6e6 (body log column 1)
    "shape_grad_halved": ("axis_zscore",),                           # 3.0e4 (betas)
    "prior_grad_0.9": ("axis_zscore", "rot6d_zscore"),               # 2.6e3 (reprojection), 6.2e3 (body log column 0)
    "rot6d_grad_not_through_rodrigues": ("rot6d_zscore", "rot6d_none", "zero_pose_rot6d"),   # 1.1e4, 1.9e3, 1.2e3 (pose)
    "noise_row_shifted": ("axis_zscore",),                           # 1.5e4 (body log column 0)
}


@pytest.mark.parametrize("fault", TL.SMPLIFY_FAULTS)
def test_a_seeded_fault_leaves_the_band(fault):
    """A kernel with this defect could not pass the GPU comparison: seeded into the float64 oracle it moves a compared quantity by more
    than 10 x the GPU tolerance, in every case listed for it."""
    for name in FAULT_CASES[fault]:
        d = SC.distances(SC.run_oracle(name, fault=fault), SC.reference(name))
        k = max(d, key=lambda q: d[q] / SC.TOL[q])
        print(f"{fault} in {name}: {k} moves {d[k]:.2e} = {d[k] / SC.TOL[k]:.1f} x its tolerance")
        assert d[k] > 10 * SC.TOL[k], (fault, name, k, d[k])


def test_the_float64_label_guard_refuses_an_ambiguous_time():
    """The sigma-table index is trunc(fp32(t) * 999) in the reference; a time whose fp64 product truncates differently is refused rather than
    silently arbitrated with another table entry."""
    cand = [float(np.float32(k) / np.float32(999.0)) for k in range(1, 999)]
    bad = [t for t in cand if int(np.float32(t) * np.float32(999)) != int(t * 999)]
    assert bad                                        # (k / 999 rounded down in fp32: the exact product is just under k, the fp32 product is k)
    with pytest.raises(ValueError):
        TL._smplify_check_label(R.SubVP(N=500), bad[0])
    for tk in SC.t_list():
        TL._smplify_check_label(R.SubVP(N=500), tk)
        TL._smplify_check_label(R.VP(N=500, discrete=True), tk)
