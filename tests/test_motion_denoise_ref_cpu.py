"""The extended motion-denoising loop of oracle/task_loops.py is checked here before it judges the kernels
(tests/test_gpu_motion_denoise.py): against the reference's own loop (golden g15), its float64 run against its unchanged default, a batch of
sequences against one run per sequence, for the distance of its float32 run from its float64 run over the GPU case matrix (the band the
GPU tolerance is 8 x of), and for sharpness -- every seeded fault leaves that tolerance."""
import numpy as np
import pytest
import torch

import motion_denoise_cases as MC
from helpers import load, rel_err
from weights import make_weights
from oracle import score_ref as R
from oracle import task_loops as TL


def _g15(tag="a", **kw):
    g, st = load("g15_motion_denoise_loop"), load("g10_normalizer")
    p = make_weights(int(g["seed"]))
    p["sigmas"] = R.sigma_table()
    out = TL.motion_denoise_optimize(p, R.SubVP(N=int(g["sde_N"])), MC.asset(), st["stats/axis_normalize2/mean_poses"],
                                     st["stats/axis_normalize2/std_poses"], g[f"{tag}_joints3d"], g["gt"], g["init"], g[f"{tag}_noise"],
                                     iterations=int(g["iterations"]), steps_per_iter=int(g["steps_per_iter"]), **kw)
    return g, out


def test_float32_oracle_reproduces_the_reference_loop():
    """Golden g15, case a, is the reference's own MotionDenoise.optimize (fp32 loop around an fp64 body-model stand-in).  The extended
    oracle with everything in float32 lands on it inside the tolerances tests/test_oracle_golden.py holds the default oracle to."""
    g, out = _g15(dtype=torch.float32, details=True)
    assert out["pose"].dtype == np.float32 and out["pose_steps"].shape == (6, 12, 63)
    assert rel_err(out["pose"], g["a_pose_final"]) < 1e-5
    assert rel_err(out["pose_steps"][-2], g["a_pose_before_last_step"]) < 1e-5
    for k in ("init_MPJPE", "MPJPE", "MPVPE"):
        assert np.allclose(out[k], g[f"a_{k}"], rtol=1e-4, atol=1e-5), k
    assert out["data_kept"].all() and (out["log"] > 0).all()


def test_float64_oracle_agrees_with_the_default():
    """The defaults are the loop the oracle always was (fp32 network and pose leaf, float64 body model, a (pose, metrics) pair): its
    details are the same run, and the all-float64 loop agrees with it to the tolerances of tests/test_oracle_golden.py."""
    _, (final, res) = _g15()
    _, full = _g15(details=True)
    _, f64 = _g15(dtype=torch.float64, details=True)
    assert final.dtype == np.float32 and np.array_equal(final, full["pose"]) and np.array_equal(final, full["pose_steps"][-1])
    assert f64["pose"].dtype == np.float64
    assert rel_err(f64["pose"], final) < 1e-5
    for k in ("init_MPJPE", "MPJPE", "MPVPE"):
        assert np.array_equal(res[k], full[k])
        assert np.allclose(f64[k], res[k], rtol=1e-4, atol=1e-5), k


def test_adam_state_and_gradients_are_those_of_the_loop():
    """grad_steps is what Adam was handed: replaying Adam on it reproduces m, v and every pose."""
    ref, x = MC.reference("axis_zscore"), MC.inputs("axis_zscore")
    m, v, pose = 0.0, 0.0, x["init"].astype(np.float64)
    for k, g in enumerate(ref["grad_steps"], start=1):
        m, v = MC.BETA1 * m + (1 - MC.BETA1) * g, MC.BETA2 * v + (1 - MC.BETA2) * g * g
        pose = pose - 0.03 / (1 - MC.BETA1 ** k) * m / (np.sqrt(v) / np.sqrt(1 - MC.BETA2 ** k) + 1e-8)
        assert np.abs(pose - ref["pose_steps"][k - 1]).max() < 1e-13
    assert np.abs(m - ref["adam_m"]).max() < 1e-13 * np.abs(m).max() and np.abs(v - ref["adam_v"]).max() < 1e-13 * np.abs(v).max()
    assert np.allclose(ref["v0"], (1 - MC.BETA2) * ref["grad0"] ** 2, rtol=1e-14, atol=0)


def test_a_batch_of_sequences_is_one_run_per_sequence():
    """frames_per_sequence = F: S independent runs of the single-sequence loop on slices of pose, observation and noise -- the prior with
    ``sum_over_batch`` and batch_size = F, as the single-sequence call gets it (include/dposer_hip.h: 1 / F in the one-call loop)."""
    name = "seq_3x8"
    c, x, ref = MC.CASES[name], MC.inputs(name), MC.reference(name)
    a, b = MC.norm_stats(c["rot"], c["norm"])
    for s in range(c["S"]):
        sl = slice(s * c["F"], (s + 1) * c["F"])
        one = TL.motion_denoise_optimize(MC.params(c["rot"]), MC.make_sde(c["kind"]), MC.asset(), a, b, x["joints3d"][sl], x["gt"][sl], x["init"][sl],
                                         x["noise"][:, sl], iterations=MC.ITERS, steps_per_iter=MC.SPI, dtype=torch.float64, details=True)
        for k in ("pose_steps", "grad_steps", "adam_m", "adam_v"):
            assert np.abs(one[k] - ref[k][..., sl, :]).max() <= 1e-12 * np.abs(one[k]).max(), (s, k)
        assert np.abs(one["log"][:, 0] - ref["log"][:, s]).max() <= 1e-12 * np.abs(one["log"]).max()
        for k in ("init_MPJPE", "MPJPE", "MPVPE"):
            assert np.abs(one[k] - ref[k][sl]).max() < 1e-10, (s, k)


def test_float32_oracle_stays_inside_the_band():
    """Every case of the GPU matrix in float32 against float64.  The maxima are the D32 constants the GPU tolerance is 8 x of: every
    case must sit inside that tolerance (torch-fp32 itself passes the test the kernels take), a fresh measurement must stay within 2 x of
    the committed constants (and they must not have been inflated: the maxima reach a quarter of them), and the inputs must be well
    conditioned: the pose of every step within 1e-5, every coordinate compared."""
    worst = {k: 0.0 for k in MC.D32}
    for name in MC.CASES:
        ref = MC.reference(name)
        d = MC.distances(MC.run_oracle(name, torch.float32), ref)
        print(name, " ".join(f"{k}={v:.2e}" for k, v in d.items()))
        assert d["pose"] <= MC.POSE_D32_MAX, (name, d["pose"])
        for k, v in d.items():
            assert v < MC.TOL[k], (name, k, v, MC.TOL[k])
            worst[k] = max(worst[k], v)
        assert ref["pose_steps"].shape == (MC.STEPS,) + MC.inputs(name)["init"].shape and np.isfinite(ref["pose_steps"]).all()
    print("d32 maxima:", " ".join(f"{k}={v:.2e}" for k, v in worst.items()))
    for k, v in worst.items():
        assert MC.D32[k] / 4 <= v <= MC.D32[k] * 2, (k, v, MC.D32[k])


def test_the_edge_cases_are_the_edges_they_claim():
    x = MC.inputs("zero_pose_rot6d")
    assert (x["init"][MC.ZERO_FRAME] == 0).all() and (np.abs(x["init"]).sum(axis=1) > 0).sum() == 11      # one zero frame: no two frames alike
    x = MC.inputs("large_angle_rot6d")
    assert np.linalg.norm(x["init"][MC.LARGE_FRAME, 3 * MC.LARGE_JOINT:3 * MC.LARGE_JOINT + 3]) > 3.0
    # the NaN observation: sequence 1 loses its data term in every step (log column 1 = 0), sequence 0 is the run it is alone
    name = "nan_observation"
    c, x, ref = MC.CASES[name], MC.inputs(name), MC.reference(name)
    assert np.isnan(x["joints3d"]).sum() == 1 and np.isnan(x["joints3d"][MC.NAN_AT])
    assert ref["data_kept"][:, 0].all() and not ref["data_kept"][:, 1].any()
    assert (ref["log"][:, 1, 1] == 0).all() and (ref["log"][:, 0, 1] > 0).all() and np.isfinite(ref["log"]).all() and np.isfinite(ref["pose"]).all()
    assert np.isnan(ref["init_MPJPE"]).sum() == 1 and np.isnan(ref["init_MPJPE"][MC.NAN_AT[0]])
    a, b = MC.norm_stats(c["rot"], c["norm"])
    sl = slice(0, c["F"])
    one = TL.motion_denoise_optimize(MC.params(c["rot"]), MC.make_sde(c["kind"]), MC.asset(), a, b, x["joints3d"][sl], x["gt"][sl], x["init"][sl],
                                     x["noise"][:, sl], iterations=MC.ITERS, steps_per_iter=MC.SPI, dtype=torch.float64, details=True)
    assert np.abs(one["pose"] - ref["pose"][sl]).max() < 1e-12
    for name in MC.CASES:
        x = MC.inputs(name)
        d = np.abs(x["init"][1:] - x["init"][:-1]).max(axis=1)
        assert d.min() > 1e-2, name                  # no two neighbouring frames alike
        assert all(np.isfinite(v).all() for k, v in x.items() if v is not None and not (name == "nan_observation" and k == "joints3d"))


# fault -> the cases it is seeded into (measured: the largest distance / tolerance over the compared quantities, and that of the
# first-step gradient -- the comparison that sees a wrongly scaled term on its own)
FAULT_CASES = {
    "temporal_crosses_sequences": ("seq_3x8", "seq_2x23"),                    # 1.3e5 (log column 0; grad0 8.0e3), 5.3e4 (grad0 9.0e3)
    "temporal_mean_over_T": ("axis_zscore", "seq_6x2"),                       # 6.5e4 (log column 0; grad0 2.8e3), 3.9e5 (grad0 2.0e4)
    "data_guard_ignored": ("nan_observation",),                               # inf: NaN poses
    "data_mean_over_frames": ("axis_zscore",),                                # 1.5e7 (log column 1; grad0 7.0e5)
    "min_max_without_2": ("axis_minmax", "rot6d_minmax"),                     # 9.5e3 (grad0), 5.8e4 (v0; grad0 5.7e4)
    "prior_grad_not_divided_by_std": ("axis_zscore", "rot6d_zscore"),         # 9.7e4 (grad0), 1.1e5 (grad0)
    "rot6d_grad_not_through_rodrigues": ("rot6d_zscore", "zero_pose_rot6d", "large_angle_rot6d"),   # 2.5e4, 4.1e4 (grad0), 3.3e4 (adam_m; grad0 2.1e4)
    "prior_weight_of_previous_iteration": ("axis_zscore",),                   # 4.6e3 (adam_m; pose 1.3e3)
    "noise_row_shifted": ("axis_zscore",),                                    # 4.8e4 (adam_v; pose 1.6e4)
    "weighted_on": ("axis_zscore",),                                          # 9.9e4 (log column 2; grad0 2.5e4)
}
# what a one-step call can see of a fault: the two below change nothing in the first step of the first outer iteration
INVISIBLE_IN_STEP_ONE = ("prior_weight_of_previous_iteration", "noise_row_shifted")


@pytest.mark.parametrize("fault", TL.MOTION_DENOISE_FAULTS)
def test_a_seeded_fault_leaves_the_band(fault):
    """A kernel with this defect could not pass the GPU comparison: seeded into the float64 oracle it moves a compared quantity out of the
    GPU tolerance (8 x d32) -- by more than 10 x that tolerance, in every case listed for it; and, where the fault acts in the first
    step, the first-step gradient alone shows it."""
    for name in FAULT_CASES[fault]:
        got = MC.run_oracle(name, fault=fault)
        del got["pose_steps"]                             # the GPU comparison sees the final pose only
        d = MC.distances(got, MC.reference(name))
        k = max(d, key=lambda q: d[q] / MC.TOL[q])
        print(f"{fault} in {name}: {k} moves {d[k]:.2e} = {d[k] / MC.TOL[k]:.3g} x its tolerance; grad0 {d['grad0'] / MC.TOL['grad0']:.3g} x, "
              f"pose {d['pose'] / MC.TOL['pose']:.3g} x")
        assert d[k] > 10 * MC.TOL[k], (fault, name, k, d[k])
        if fault not in INVISIBLE_IN_STEP_ONE:
            assert d["grad0"] > 10 * MC.TOL["grad0"], (fault, name, d["grad0"])
