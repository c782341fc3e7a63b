"""The one-call motion-denoising loop with PARTIAL observations -- joints_conf / obs_joints, k_md_joint_obs in csrc/tasks.hip -- against the
float64 reference of tests/md_partial_ref.py, case by case and quantity by quantity: the final pose, the first step's gradient and second
moment (from a one-step call), Adam's state, every step, sequence and column of the loss log, the kept / dropped decision of every step and
sequence, and the five metrics.  tests/md_partial_cases.py holds the cases and the band (8 x the float32 reference's distance from the
float64 reference); tests/test_md_partial_ref_cpu.py checks that reference and shows that six seeded faults leave the band."""
import numpy as np
import pytest
import torch

import md_partial_cases as PC
import motion_denoise_cases as MC
from gpu_common import DEV, make_model, t2n
from helpers import _log_measured

pytestmark = pytest.mark.gpu


def _md(name):
    from dposer_amd.body_model.body_model import BodyModel
    from dposer_amd.dataset.AMASS import Posenormalizer
    from dposer_amd.tasks.motion_denoising import MotionDenoise
    c = PC.CASES[name]
    cfg, m, _ = make_model(MC.SEED, D=63 if c["rot"] == "axis" else 126, precision="fp32", embedding="positional")
    bm = BodyModel(MC.asset()).to(DEV)

    class Args:
        device = DEV

    nz = Posenormalizer({k: torch.tensor(v) for k, v in MC.stats(c["rot"]).items()}, device=DEV, normalize=True, min_max=False, rot_rep=c["rot"])
    md = MotionDenoise(cfg, Args(), m, bm, sde_N=PC.SDE_N, batch_size=c["F"], normalizer=nz)
    assert md._fused_supported()
    return md


def _call(md, name, iterations, steps_per_iter, noise, strategy="3", conf="case", fused=True):
    """One ``optimize`` (one sequence) / ``optimize_sequences`` (S > 1) call; ``conf``: 'case' = the case's confidences, else what to pass."""
    c, x = PC.CASES[name], PC.inputs(name)
    S, F = c["S"], c["F"]
    d = lambda a: None if a is None else torch.tensor(a, device=DEV)
    n_obs = x["joints3d"].shape[1]
    cf = d(x["conf"]) if isinstance(conf, str) else conf
    kw = dict(time_strategy=strategy, sample_time=PC.SAMPLE_TIME, iterations=iterations, steps_per_iter=steps_per_iter,
              noise=d(np.ascontiguousarray(noise, dtype=np.float32)), obs_joints=x["rows"])
    if S == 1:
        res = md.optimize(d(x["joints3d"]), gt_poses=d(x["gt"]), init_poses=d(x["init"]), fused=fused, joints_conf=cf, **kw)
    else:
        res = md.optimize_sequences(d(x["joints3d"]).reshape(S, F, n_obs, 3), d(x["gt"]).reshape(S, F, 63), init_poses=d(x["init"]).reshape(S, F, 63),
                                    joints_conf=None if cf is None else cf.reshape(S, F, n_obs), **kw)
    out = {k: np.asarray(res[k]).reshape(-1) for k in res if k != "pose_body"}
    out["pose"] = t2n(res["pose_body"]).reshape(S * F, 63)
    if fused:
        assert tuple(md.loss_log.shape) == (iterations * steps_per_iter, S, 3)
        out.update(log=t2n(md.loss_log), adam_m=t2n(md.adam_state[0]), adam_v=t2n(md.adam_state[1]))
    return out


def _run_case(md, name, **kw):
    """A one-step call at the fixed time of strategy '2' -- the gradient is m / (1 - beta1), its square v / (1 - beta2) -- then the whole run."""
    z = PC.inputs(name)["noise"]
    one = _call(md, name, 1, 1, z[:1], strategy="2", **kw)
    got = _call(md, name, PC.ITERS, PC.SPI, z, **kw)
    got["grad0"], got["v0"] = one["adam_m"] / (1 - PC.BETA1), one["adam_v"]
    return got


def _hold_to(got, ref, what):
    dist = PC.distances(got, ref, log_prior_is_total=True)
    ratio, k = PC.worst_ratio(dist)
    _log_measured("d32_ratio", ratio)
    print(f"{what}: worst {k} = {dist[k]:.2e} = {ratio:.2f} x d32 | " + " ".join(f"{q}={v / PC.D32[q]:.2f}" for q, v in dist.items()))
    assert np.isfinite(got["pose"]).all() and np.isfinite(got["log"]).all()
    for q, v in dist.items():
        assert v < PC.TOL[q], (what, q, v, PC.TOL[q])
    # the data-term decision of every step and sequence (a dropped term is logged as 0), and one prior value per step: the batch total
    assert np.array_equal(got["log"][:, :, 1] != 0, ref["data_kept"])
    assert (got["log"][:, :, 2] == got["log"][:, :1, 2]).all()
    return ratio


@pytest.mark.parametrize("name", list(PC.CASES))
def test_partial_observations_match_the_float64_reference_quantity_by_quantity(name):
    """Every case of tests/md_partial_cases.py through ``optimize`` (one sequence) / ``optimize_sequences``: explicit ones; the left leg
    occluded with NaN under c = 0 (axis-angle 2 x 6, rot6d 1 x 12); fractional confidences at 3 x 8, 2 x 23 (506 entries per sequence: two
    trips of the stride loop, a sequence boundary inside a workgroup of four poses) and 6 x 2; a joint list without confidences (head and
    wrists) and an unsorted one with them; a sequence without a live entry (dropped and logged 0 in every step, the other untouched); ~30 %
    dead entries under 0, negative and NaN confidences with one frame fully dead; a NaN under c = 1 (the term is dropped, as without
    confidences).  Tolerance per quantity: 8 x the float32 reference's distance from the float64 reference (PC.D32 / PC.TOL).
    Measured on an MI355X, the worst GPU distance / d32 over the thirteen quantities of each case (the tolerance is 8): ones_1x12 0.98
    (adam_m), left_leg_nan_2x6 1.39 (MPVPE), fractional_3x8 0.94 (log_1), fractional_2x23 1.30 (MPJPE), sparse3_2x23 1.53 (adam_m),
    unsorted_rows_1x12 1.50 (adam_m), blind_sequence_2x6 0.78 (v0), frame_dropout_2x6 1.15 (adam_m), nan_visible_2x6 0.94 (log_0),
    rot6d_left_leg_1x12 1.08 (v0), tiny_6x2 0.99 (log_0).  The final pose is at 0.21 ... 0.57, the data column of the log at 0.36 ... 0.96,
    the observed / unobserved split at 0.24 ... 0.99 everywhere.  Every ratio is logged (DPOSER_LOG_ERR) and printed."""
    ref = PC.reference(name)
    got = _run_case(_md(name), name)
    _hold_to(got, ref, name)
    if name == "blind_sequence_2x6":
        assert (got["log"][:, 1, 1] == 0).all() and (got["log"][:, 0, 1] > 0).all()
    if name == "frame_dropout_2x6":
        assert np.isnan(got["init_MPJPE"][PC.DEAD_FRAME]) and np.isnan(got["MPJPE_observed"][PC.DEAD_FRAME])


@pytest.mark.parametrize("home", ["0", "1", "2"])
@pytest.mark.parametrize("name", ["fractional_2x23", "left_leg_nan_2x6"])
def test_every_home_of_the_temporal_gradient_takes_partial_observations(name, home, tuning_env):
    """k_md_joint_obs in front of each of the three homes of the temporal gradient: k_md_vert_grad (0), dposer_lbs_forward_temporal_grad (1)
    and dposer_lbs_backward_temporal (2: the log form with n_temp_part = 0, column 0 filled by k_md_temp_log afterwards; gradient rows
    read with the joint-row stride).
    Measured, worst distance / d32: fractional_2x23 1.26 (MPJPE) in homes 0 and 1, which carry the same bits, 1.22 in home 2 (the data
    column 0.73, the pose 0.41 in all three); left_leg_nan_2x6 1.27 (MPVPE) in every home (the data column 0.55 / 0.55 / 0.58)."""
    from dposer_amd import _C
    md = _md(name)
    tuning_env(DPOSER_MD_FUSED_TEMPORAL=home, DPOSER_LBS_JOINT_STREAM_MIN="1")
    if home == "2":
        md.body_model.bm.joint_csr()
        assert _C.lib().dposer_lbs_temporal_in_backward_ok(md.body_model.bm._handle(), 4, PC.CASES[name]["S"] * PC.CASES[name]["F"]) == 1
    _hold_to(_run_case(md, name), PC.reference(name), f"{name} home {home}")


def test_explicit_ones_through_the_new_kernel_match_the_plain_call():
    """c = 1 and rows = 0 .. 21 passed EXPLICITLY run k_md_joint_obs; joints_conf = None, obs_joints = None run k_md_joint.  Same inputs:
    the two stay inside the band of each other (by construction they carry the same bits: the weight sum is the entry count, exactly),
    and both inside the band of the float64 reference.
    Measured: pose, Adam's state, the three log columns, MPJPE and MPVPE differ by exactly 0; init_MPJPE by 9.5e-7 cm (0.43 x d32: the
    masked mean of the partial metrics against torch.mean)."""
    name = "ones_1x12"
    x, z = PC.inputs(name), PC.inputs(name)["noise"]
    d = lambda a: torch.tensor(a, device=DEV)
    ones = _run_case(_md(name), name)
    md = _md(name)
    kw = dict(time_strategy="3", sample_time=PC.SAMPLE_TIME, iterations=PC.ITERS, steps_per_iter=PC.SPI, noise=d(z), fused=True)
    res = md.optimize(d(x["joints3d"]), gt_poses=d(x["gt"]), init_poses=d(x["init"]), **kw)
    assert sorted(res) == ["MPJPE", "MPVPE", "init_MPJPE", "pose_body"]          # neither argument: the dict of every call before them
    plain = {k: np.asarray(res[k]).reshape(-1) for k in ("init_MPJPE", "MPJPE", "MPVPE")}
    plain.update(pose=t2n(res["pose_body"]), log=t2n(md.loss_log), adam_m=t2n(md.adam_state[0]), adam_v=t2n(md.adam_state[1]))
    rows = md.optimize(d(x["joints3d"]), gt_poses=d(x["gt"]), init_poses=d(x["init"]), obs_joints=list(range(22)),
                       joints_conf=torch.ones(12, 22, device=DEV), **kw)
    dist = MC.distances(dict(ones, **{k: ones[k] for k in plain}), plain)
    dist = {k: v for k, v in dist.items() if k not in ("grad0", "v0")}
    print("explicit ones vs None:", " ".join(f"{q}={v:.2e}" for q, v in dist.items()))
    for q, v in dist.items():
        assert v < PC.TOL[q], (q, v)
    assert np.abs(t2n(rows["pose_body"]) - plain["pose"]).max() < PC.TOL["pose"]
    _log_measured("ones_vs_none_pose", dist["pose"])


def test_the_step_by_step_torch_path_applies_the_same_rule():
    """fused=False: the rule in torch (MotionDenoise._partial_data_term) through autograd and torch.optim.Adam, on the unsorted joint list
    with fractional confidences: pose and metrics inside the band of the float64 reference, so both paths stay interchangeable.
    Measured, distance / d32: pose 0.21, init_MPJPE 0.50, MPJPE 0.58, MPVPE 0.66, MPJPE_observed 0.37, MPJPE_unobserved 0.37."""
    name = "unsorted_rows_1x12"
    ref = PC.reference(name)
    got = _call(_md(name), name, PC.ITERS, PC.SPI, PC.inputs(name)["noise"], fused=False)
    worst = 0.0
    for q in ("pose",) + PC.METRICS:
        v = MC._absmax(got[q], ref[q])
        worst = max(worst, v / PC.D32[q])
        print(f"{q}: {v:.2e} = {v / PC.D32[q]:.2f} x d32")
        assert v < PC.TOL[q], (q, v, PC.TOL[q])
    _log_measured("d32_ratio", worst)


def test_the_torch_path_survives_dead_and_dropped_terms():
    """fused=False on one sequence each of: NaN under c = 0 (left leg), no live entry at all, and a NaN under c = 1 (term dropped): the pose
    stays finite -- a masked NaN must give an exact 0 gradient, not 0 x NaN -- and matches the one-call loop's inside the band."""
    for name, seq in (("left_leg_nan_2x6", 0), ("blind_sequence_2x6", 1), ("nan_visible_2x6", 1)):
        c, x = PC.CASES[name], PC.inputs(name)
        sl = slice(seq * c["F"], (seq + 1) * c["F"])
        d = lambda a: torch.tensor(a, device=DEV)
        out = []
        for fused in (True, False):
            md = _md(name)
            res = md.optimize(d(x["joints3d"][sl]), gt_poses=d(x["gt"][sl]), init_poses=d(x["init"][sl]), joints_conf=d(x["conf"][sl]), fused=fused,
                              time_strategy="3", iterations=PC.ITERS, steps_per_iter=PC.SPI, noise=d(np.ascontiguousarray(x["noise"][:, sl])))
            out.append(t2n(res["pose_body"]))
        assert np.isfinite(out[1]).all(), name
        assert np.abs(out[0] - out[1]).max() < PC.TOL["pose"], (name, np.abs(out[0] - out[1]).max())
        assert np.abs(out[0] - PC.reference(name)["pose"][sl]).max() < PC.TOL["pose"], name


def test_the_dataset_loop_averages_every_metric_over_the_frames_that_have_it():
    """evaluate_motion_denoising with occlude_joints('left_leg') plus one fully dead frame on 4 sequences of 6 frames, two per call: the
    returned names are fixed, and every mean equals the mean of optimize_sequences' per-frame values over the non-NaN frames."""
    from dposer_amd.tasks.motion_denoising import evaluate_motion_denoising
    from dposer_amd.utils.misc import occlude_joints
    name = "left_leg_nan_2x6"
    x = PC.inputs(name)
    d = lambda a: torch.tensor(a, device=DEV)
    S, F = 4, 6
    clean = np.where(np.isnan(x["joints3d"]), 0.0, x["joints3d"]).astype(np.float32)
    j = d(np.concatenate([clean, clean[::-1]]).reshape(S, F, 22, 3))
    gt = d(np.concatenate([x["gt"], x["gt"][::-1]]).reshape(S, F, 63))
    j, conf = occlude_joints(j, part="left_leg")
    conf[2, 3] = 0.0                                         # one frame without a live entry: no init_MPJPE, nothing observed
    # (the recorded noise of two sequences serves every call of two; every sequence starts from the module's own initial poses)
    kw = dict(time_strategy="3", iterations=1, steps_per_iter=2, noise=d(np.ascontiguousarray(x["noise"][:2])))
    md = _md(name)
    means, n = evaluate_motion_denoising(md, j, gt, sequences_per_call=2, num_replicas=1, rank=0, joints_conf=conf, **kw)
    assert n == S and list(means) == ["MPJPE", "MPVPE", "init_MPJPE", "MPJPE_observed", "MPJPE_unobserved"]
    parts = [md.optimize_sequences(j[s:s + 2], gt[s:s + 2], joints_conf=conf[s:s + 2], **kw) for s in (0, 2)]
    for k, v in means.items():
        per_frame = np.concatenate([np.asarray(p[k]).reshape(-1) for p in parts])
        assert per_frame.shape == (S * F,)
        assert np.isnan(per_frame).sum() == (1 if k in ("init_MPJPE", "MPJPE_observed") else 0), k
        assert np.isfinite(v) and abs(v - np.nanmean(per_frame.astype(np.float64))) < 1e-9 * max(1.0, abs(v)), (k, v)


def test_host_checks_and_vis_refusal_on_the_device_path():
    name = "sparse3_2x23"
    md, x = _md(name), PC.inputs(name)
    d = lambda a: torch.tensor(a, device=DEV)
    j, gt = d(x["joints3d"][:23]), d(x["gt"][:23])
    with pytest.raises(ValueError):
        md.optimize(j, gt_poses=gt, obs_joints=[15, 20, 55], iterations=1, steps_per_iter=1)          # 55 is no tree joint of SMPL-X
    with pytest.raises(NotImplementedError):
        md.out_path = "unused"
        md.optimize(j, gt_poses=gt, obs_joints=[15, 20, 21], vis=True, iterations=1, steps_per_iter=1)
