"""The float64 reference of the motion-denoising loop with partial observations (tests/md_partial_ref.py) is checked here before it judges
the kernels (tests/test_gpu_md_partial.py): against oracle/task_loops.motion_denoise_optimize where the two must coincide, for the distance
of its float32 run from its float64 run over the case matrix (the band the GPU tolerance is 8 x of) and for sharpness -- every seeded
fault leaves that tolerance.  Also the host side of the feature that needs no GPU: the argument checks, occlude_joints and the two
fields appended to the argument structure."""
import os
import shutil
import subprocess
import types

import numpy as np
import pytest
import torch

import md_partial_cases as PC
import md_partial_ref as PR
import motion_denoise_cases as MC
from oracle import task_loops as TL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ones_and_no_list_is_the_oracle_loop():
    """ones_1x12 (c = 1, rows = None) in float64 against oracle/task_loops.motion_denoise_optimize on the same inputs: the two differ by the
    order of one 264-term sum and the clamp at 1e-36 (never active here), i.e. by float64 rounding.  Every compared quantity below
    D32 / 1000.  Measured: init_MPJPE 1.8e-15 cm (numpy's norm against torch's sqrt of a sum); every other quantity -- pose, grad0, v0,
    Adam's state, the three log columns, MPJPE, MPVPE -- exactly 0: with c = 1 torch forms the same sum."""
    name = "ones_1x12"
    x, new = PC.inputs(name), PC.reference(name)
    assert (x["conf"] == 1).all() and x["rows"] is None
    a, b = MC.norm_stats("axis", "zscore")
    run = lambda it, spi, z, strategy: TL.motion_denoise_optimize(
        MC.params("axis"), MC.make_sde("subvp"), MC.asset(), a, b, x["joints3d"], x["gt"], x["init"], z, iterations=it, steps_per_iter=spi,
        dtype=torch.float64, time_strategy=strategy, sample_time=PC.SAMPLE_TIME, frames_per_sequence=12, details=True)
    old = run(PC.ITERS, PC.SPI, x["noise"], "3")
    one = run(1, 1, x["noise"][:1], "2")
    old["grad0"], old["v0"] = one["grad_steps"][0], one["adam_v"]
    d = MC.distances(new, old)
    print(" ".join(f"{k}={v:.1e}" for k, v in d.items()))
    for k, v in d.items():
        assert v < PC.D32[k] / 1000, (k, v)
    assert np.array_equal(new["data_kept"], old["data_kept"]) and new["data_kept"].all()
    # all 22 joints observed: the observed split is MPJPE itself, the unobserved set is empty in every frame
    assert np.array_equal(new["MPJPE_observed"], new["MPJPE"]) or np.abs(new["MPJPE_observed"] - new["MPJPE"]).max() < 1e-12
    assert np.isnan(new["MPJPE_unobserved"]).all()


def test_float32_reference_stays_inside_the_band():
    """Every case in float32 against float64.  The maxima are the D32 constants the GPU tolerance is 8 x of: every case sits inside that
    tolerance, a fresh measurement stays within 2 x of the committed constants (which are not inflated: the maxima reach a quarter of
    them), and the seeds are well conditioned: the pose of every step within 1e-5, every coordinate compared.  The kept / dropped
    decisions of the two precisions coincide."""
    worst = {k: 0.0 for k in PC.D32}
    for name in PC.CASES:
        ref = PC.reference(name)
        got = PC.run_reference(name, torch.float32)
        d = PC.distances(got, ref)
        print(name, " ".join(f"{k}={v:.2e}" for k, v in d.items()))
        assert d["pose"] <= PC.POSE_D32_MAX, (name, d["pose"])
        assert np.array_equal(got["data_kept"], ref["data_kept"]), name
        for k, v in d.items():
            assert v < PC.TOL[k], (name, k, v, PC.TOL[k])
            worst[k] = max(worst[k], v)
        assert ref["pose_steps"].shape == (PC.STEPS,) + PC.inputs(name)["init"].shape and np.isfinite(ref["pose_steps"]).all()
    print("d32 maxima:", " ".join(f"{k}={v:.2e}" for k, v in worst.items()))
    for k, v in worst.items():
        assert PC.D32[k] / 4 <= v <= PC.D32[k] * 2, (k, v, PC.D32[k])


def test_the_cases_are_the_edges_they_claim():
    for name, c in PC.CASES.items():
        x = PC.inputs(name)
        T = c["S"] * c["F"]
        n_obs = 22 if c["rows"] is None else len(c["rows"])
        assert x["joints3d"].shape == (T, n_obs, 3) and (x["conf"] is None or x["conf"].shape == (T, n_obs))
        live = np.ones((T, n_obs), bool) if x["conf"] is None else x["conf"] > 0
        nan = np.isnan(x["joints3d"]).any(axis=2)
        if name != "nan_visible_2x6":
            assert not (nan & live).any(), name                       # a NaN sits under a dead entry only
        assert np.abs(x["init"][1:] - x["init"][:-1]).max(axis=1).min() > 1e-2, name      # no two neighbouring frames alike
    assert PC.CASES["fractional_2x23"]["F"] * 22 == 506 > 256 and 23 * 3 == 69 < 256
    x = PC.inputs("left_leg_nan_2x6")
    assert np.isnan(x["joints3d"][:, list(PC.LEFT_LEG)]).all() and (x["conf"][:, list(PC.LEFT_LEG)] == 0).all() and x["conf"].sum() == 12 * 18
    x = PC.inputs("fractional_3x8")
    assert x["conf"].min() >= 0.2 and x["conf"].max() <= 1.0 and len(np.unique(x["conf"])) > 500
    # the blind sequence: dropped and logged 0 in every step, and sequence 0 is the run it is alone
    name = "blind_sequence_2x6"
    c, x, ref = PC.CASES[name], PC.inputs(name), PC.reference(name)
    assert (x["conf"][6:] == 0).all() and (x["conf"][:6] == 1).all()
    assert ref["data_kept"][:, 0].all() and not ref["data_kept"][:, 1].any() and (ref["log"][:, 1, 1] == 0).all()
    assert np.isfinite(ref["pose"]).all() and np.abs(ref["pose"][6:] - x["init"][6:]).max() > 1e-2          # it keeps moving: prior and temporal term
    a, b = MC.norm_stats("axis", "zscore")
    alone = PR.motion_denoise_partial(MC.params("axis"), MC.make_sde("subvp"), MC.asset(), a, b, x["joints3d"][:6], x["gt"][:6], x["init"][:6],
                                      x["noise"][:, :6], joints_conf=x["conf"][:6], iterations=PC.ITERS, steps_per_iter=PC.SPI)
    assert np.abs(alone["pose"] - ref["pose"][:6]).max() < 1e-12
    assert np.isnan(ref["init_MPJPE"][6:]).all() and np.isnan(ref["MPJPE_observed"][6:]).all() and np.isfinite(ref["MPJPE_unobserved"][6:]).all()
    # the dropout case: the three ways of not being live, one frame fully dead, and a real observed / unobserved split
    x, ref = PC.inputs("frame_dropout_2x6"), PC.reference("frame_dropout_2x6")
    cf = x["conf"]
    dead = ~(cf > 0)
    assert 0.2 < dead.mean() < 0.45 and dead[PC.DEAD_FRAME].all() and (cf == 0).any() and (cf < 0).any() and np.isnan(cf).any()
    assert np.isnan(x["joints3d"][dead]).all() and len({tuple(r) for r in dead}) == 12                  # differently in every frame
    assert np.isnan(ref["init_MPJPE"]).sum() == 1 and np.isnan(ref["init_MPJPE"][PC.DEAD_FRAME]) and np.isnan(ref["MPJPE_observed"][PC.DEAD_FRAME])
    assert np.isfinite(ref["MPJPE_unobserved"]).all() and ref["data_kept"].all()
    # a NaN under c = 1 drops the term, as without confidences
    x, ref = PC.inputs("nan_visible_2x6"), PC.reference("nan_visible_2x6")
    assert np.isnan(x["joints3d"]).sum() == 1 and x["conf"][PC.NAN_AT[:2]] == 1
    assert ref["data_kept"][:, 0].all() and not ref["data_kept"][:, 1].any() and np.isfinite(ref["pose"]).all()


# fault -> the cases it is seeded into, with the measured largest distance / tolerance over the compared quantities
FAULT_CASES = {
    "conf_ignored": ("fractional_3x8", "tiny_6x2"),
    "mean_over_count": ("fractional_3x8", "left_leg_nan_2x6"),
    "grad_unweighted": ("fractional_3x8", "tiny_6x2"),
    "nan_under_zero_poisons": ("left_leg_nan_2x6", "rot6d_left_leg_1x12"),
    "rows_as_prefix": ("sparse3_2x23", "unsorted_rows_1x12"),
    "blind_keeps_term": ("blind_sequence_2x6",),
}


@pytest.mark.parametrize("fault", PR.FAULTS)
def test_a_seeded_fault_leaves_the_band(fault):
    """A kernel with this defect could not pass the GPU comparison: seeded into the float64 reference it moves a compared quantity out of
    the GPU tolerance (8 x d32) by more than 10 x that tolerance, in every case listed for it.  Measured, the quantity that moves most
    and its distance / tolerance (the first-step gradient in brackets):
      conf_ignored            fractional_3x8 MPJPE 2.4e4 (grad0 7.3e3), tiny_6x2 log_1 4.2e4 (grad0 1.1e4)
      mean_over_count         fractional_3x8 log_1 3.3e5 (grad0 9.9e3), left_leg_nan_2x6 log_1 1.4e5 (grad0 4.4e3)
      grad_unweighted         fractional_3x8 MPJPE 4.5e4 (grad0 1.4e4), tiny_6x2 MPVPE 6.7e4 (grad0 1.9e4)
      nan_under_zero_poisons  left_leg_nan_2x6 log_1 7.8e5 (a term logged 0 where a value belongs; grad0 2.4e4), rot6d_left_leg_1x12 log_1 7.8e5 (grad0 1.3e4)
      rows_as_prefix          sparse3_2x23 log_1 1.6e6 (grad0 4.6e4), unsorted_rows_1x12 log_1 2.2e6 (grad0 1.9e5)
      blind_keeps_term        blind_sequence_2x6 log_1 7.6e5 (grad0 2.2e4)"""
    for name in FAULT_CASES[fault]:
        got = PC.run_reference(name, fault=fault)
        del got["pose_steps"]                             # the GPU comparison sees the final pose only
        d = PC.distances(got, PC.reference(name))
        k = max(d, key=lambda q: d[q] / PC.TOL[q])
        print(f"{fault} in {name}: {k} moves {d[k]:.2e} = {d[k] / PC.TOL[k]:.3g} x its tolerance; grad0 {d['grad0'] / PC.TOL['grad0']:.3g} x, "
              f"pose {d['pose'] / PC.TOL['pose']:.3g} x")
        assert d[k] > 10 * PC.TOL[k], (fault, name, k, d[k])
        assert d["grad0"] > 10 * PC.TOL["grad0"], (fault, name, d["grad0"])


def _bare_module():
    """A MotionDenoise without network and body model: the argument checks run before either is touched."""
    from dposer_amd.tasks.motion_denoising import MotionDenoise
    md = object.__new__(MotionDenoise)
    md.body_model, md.out_path = types.SimpleNamespace(bm=types.SimpleNamespace(J=55)), None
    return md


def test_host_checks_of_obs_joints_and_joints_conf():
    md = _bare_module()
    j3, j22, gt = torch.zeros(6, 3, 3), torch.zeros(6, 22, 3), torch.zeros(6, 63)
    for bad, what in (([15, 20], "names 2 joints"), ([15, 20, 20], "distinct"), ([15, 20, 55], "tree joints"), ([-1, 20, 21], "tree joints")):
        with pytest.raises(ValueError, match=what):
            md.optimize(j3, gt_poses=gt, obs_joints=bad)
        with pytest.raises(ValueError, match=what):
            md.optimize_sequences(j3[None], gt[None], obs_joints=bad)
    for shape in ((6, 21), (5, 22), (6, 22, 1), (22,)):
        with pytest.raises(ValueError, match="joints_conf must be"):
            md.optimize(j22, gt_poses=gt, joints_conf=torch.ones(shape))
    for shape in ((2, 6, 21), (3, 6, 22), (6, 21)):
        with pytest.raises(ValueError, match="joints_conf must be"):
            md.optimize_sequences(torch.zeros(2, 6, 22, 3), torch.zeros(2, 6, 63), joints_conf=torch.ones(shape))
    md.out_path = "unused"
    with pytest.raises(NotImplementedError, match="partial"):
        md.optimize(j22, gt_poses=gt, joints_conf=torch.ones(6, 22), vis=True)
    from dposer_amd.tasks.motion_denoising import _partial_observation
    conf, rows = _partial_observation(torch.zeros(2, 6, 3, 3), torch.full((6, 3), 0.5), (15, 20, 21), 55)      # [F, n_obs] is shared by the sequences
    assert conf.shape == (2, 6, 3) and conf.is_contiguous() and rows == [15, 20, 21]
    assert _partial_observation(j22, None, None, 55) == (None, None)


def test_partial_metrics_of_the_module_are_those_of_the_reference():
    """MotionDenoise's torch metrics (_partial_metrics) against the reference's numpy ones on the dropout case: same values, same NaN frames."""
    from dposer_amd.tasks.motion_denoising import _partial_metrics
    rs = np.random.RandomState(0)
    for name in ("frame_dropout_2x6", "unsorted_rows_1x12", "sparse3_2x23"):
        x = PC.inputs(name)
        T = x["gt"].shape[0]
        j_gt, j_out = rs.standard_normal((T, 55, 3)), rs.standard_normal((T, 55, 3))
        want = PR.partial_metrics(x["joints3d"].astype(np.float64), x["conf"], x["rows"], j_gt, j_out)
        got = _partial_metrics(torch.tensor(x["joints3d"], dtype=torch.float64), None if x["conf"] is None else torch.tensor(x["conf"]), x["rows"],
                               torch.tensor(j_gt), torch.tensor(j_out))
        for k in want:
            assert MC._absmax(got[k].numpy(), want[k]) < 1e-10 if not np.isnan(want[k]).all() else np.isnan(got[k].numpy()).all(), (name, k)


def test_occlude_joints_against_the_body_part_tables():
    from dposer_amd.body_model.utils import BodyPartIndices
    from dposer_amd.utils.misc import occlude_joints
    j = torch.randn(2, 5, 22, 3)
    parts = list(vars(BodyPartIndices))
    assert "left_leg" in parts and len(parts) >= 5
    for part in parts:
        out, conf = occlude_joints(j, part=part)
        hit = np.zeros(22, bool)
        hit[np.array(getattr(BodyPartIndices, part)) + 1] = True          # pose index i rotates tree joint i + 1
        assert out.shape == j.shape and conf.shape == (2, 5, 22) and conf.dtype == j.dtype
        assert torch.isnan(out[:, :, hit]).all() and torch.equal(out[:, :, ~hit], j[:, :, ~hit])
        assert (conf[:, :, hit] == 0).all() and (conf[:, :, ~hit] == 1).all()
        assert not hit[0]                                                  # no body part holds the pelvis
    assert np.array_equal(np.nonzero((occlude_joints(j, part="left_leg")[1][0, 0] == 0).numpy())[0], [1, 4, 7, 10])
    out, conf = occlude_joints(j[0], joints=[0, 21])
    assert np.array_equal(np.nonzero((conf[0] == 0).numpy())[0], [0, 21]) and torch.isnan(out[:, [0, 21]]).all() and torch.isfinite(j).all()
    out, conf = occlude_joints(j[0], part="left_leg", joints=[15])
    assert np.array_equal(np.nonzero((conf[0] == 0).numpy())[0], [1, 4, 7, 10, 15])
    with pytest.raises(ValueError):
        occlude_joints(j)
    with pytest.raises(ValueError):
        occlude_joints(j, joints=[22])


def test_the_appended_fields_close_the_argument_structure(tmp_path):
    """joints_conf and obs_rows are the LAST two fields of _C.MotionDenoiseArgs, in that order, behind rot6d; size and their offsets match
    the header's struct as the host compiler lays it out; the ABI version is still 1."""
    import ctypes as C
    from dposer_amd import _C
    names = [n for n, _ in _C.MotionDenoiseArgs._fields_]
    assert names[-3:] == ["rot6d", "joints_conf", "obs_rows"]
    assert all(t is C.c_void_p for _, t in _C.MotionDenoiseArgs._fields_[-2:])
    assert _C.MotionDenoiseArgs().joints_conf is None and _C.MotionDenoiseArgs().obs_rows is None          # unset = NULL = today's kernel
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc is not None, "the layout check needs the host C compiler"
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dposer_hip.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %d\\n", sizeof(dposer_motion_denoise_args), offsetof(dposer_motion_denoise_args, rot6d),\n'
                   '         offsetof(dposer_motion_denoise_args, joints_conf), offsetof(dposer_motion_denoise_args, obs_rows), DPOSER_ABI_VERSION);\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.check_call([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    size, o_rot, o_conf, o_rows, abi = (int(v) for v in subprocess.check_output([str(exe)], text=True).split())
    ct = _C.MotionDenoiseArgs
    assert (size, o_rot, o_conf, o_rows) == (C.sizeof(ct), ct.rot6d.offset, ct.joints_conf.offset, ct.obs_rows.offset)
    assert o_rot < o_conf < o_rows and o_rows + 8 == size and abi == 1
