"""The cases, the float64 references and the comparison band of the motion-denoising loop with PARTIAL observations (joints_conf /
obs_joints) -- shared by tests/test_md_partial_ref_cpu.py (which checks the reference of tests/md_partial_ref.py and measures the band) and
tests/test_gpu_md_partial.py (which holds the kernels to it).  Test infrastructure in the style of tests/motion_denoise_cases.py, whose
asset, weights, statistics, SDE and distance functions it uses; no GPU.

Every case is 2 outer iterations of 3 Adam steps on the synthetic SMPL-X asset with sde_N = 500, sub-VP, z-score statistics of g10,
positional embedding, recorded prior noise: distinct toy poses as the ground truth, initial poses = ground truth + 0.05 noise, observed
joints = the ground truth's joints (of the observed rows) + 0.04 noise.
"""
import functools

import numpy as np
import torch

import md_partial_ref as PR
import motion_denoise_cases as MC
from helpers import load
from oracle import fk_torch

ITERS, SPI, SDE_N, STEPS, BETA1, BETA2, SAMPLE_TIME = MC.ITERS, MC.SPI, MC.SDE_N, MC.STEPS, MC.BETA1, MC.BETA2, MC.SAMPLE_TIME

# ---- the band.  D32: the distance of the float32 reference from the float64 reference, the maximum over CASES, in the units of
# motion_denoise_cases.distances (pose and metrics: largest absolute difference, metrics in cm; grad0 / v0 / adam_m / adam_v: relative to
# the tensor's largest magnitude; log_c: relative to the column's largest entry) -- MEASURED by
# tests/test_md_partial_ref_cpu.py::test_float32_reference_stays_inside_the_band, which prints every case and asserts a fresh measurement
# within 2 x of these constants.  TOL = 8 x D32: the project's factor and reasoning (tests/smplify_cases.py).
D32 = {
    "pose": 1.9e-6,               # measured 1.85e-6 (rot6d_left_leg_1x12)
    "grad0": 1.2e-6,              # measured 1.16e-6 (rot6d_left_leg_1x12)
    "v0": 1.5e-6,                 # measured 1.47e-6 (left_leg_nan_2x6)
    "adam_m": 1.1e-6,             # measured 1.02e-6 (ones_1x12)
    "adam_v": 1.5e-6,             # measured 1.49e-6 (unsorted_rows_1x12)
    "log_0": 1.4e-7,              # measured 1.40e-7 (tiny_6x2)
    "log_1": 1.6e-7,              # measured 1.54e-7 (fractional_2x23)
    "log_2": 2.1e-7,              # measured 2.07e-7 (nan_visible_2x6)
    "init_MPJPE": 2.2e-6,         # measured 2.18e-6 (sparse3_2x23), cm
    "MPJPE": 1.4e-6,              # measured 1.37e-6 (sparse3_2x23), cm
    "MPVPE": 7.7e-6,              # measured 7.66e-6 (rot6d_left_leg_1x12), cm: the mean over 10475 vertex distances of ~10 cm
    "MPJPE_observed": 2.5e-6,     # measured 2.46e-6 (sparse3_2x23), cm: a mean over three joints
    "MPJPE_unobserved": 2.4e-6,   # measured 2.31e-6 (rot6d_left_leg_1x12), cm: a mean over four joints
}
TOL_FACTOR = 8.0
TOL = {k: TOL_FACTOR * v for k, v in D32.items()}
POSE_D32_MAX = MC.POSE_D32_MAX      # the condition on the seeds: the float32 reference's pose within 1e-5 of the float64 one's after every step
METRICS = ("init_MPJPE", "MPJPE", "MPVPE", "MPJPE_observed", "MPJPE_unobserved")
LEFT_LEG = (1, 4, 7, 10)            # BodyPartIndices.left_leg + 1: pose index i rotates tree joint i + 1


def _case(S=1, F=12, rot="axis", kind="ones", rows=None, seed=0):
    return dict(S=S, F=F, rot=rot, kind=kind, rows=rows, seed=seed)


CASES = {
    "ones_1x12": _case(),                                                   # c = 1, rows = None: the oracle's own loop through the new rule
    "left_leg_nan_2x6": _case(S=2, F=6, kind="left_leg"),                   # occlude_joints('left_leg'): NaN under c = 0 in every frame
    "fractional_3x8": _case(S=3, F=8, kind="fractional"),                   # c uniform in [0.2, 1] per entry
    "fractional_2x23": _case(S=2, F=23, kind="fractional"),                 # 506 entries per sequence: two trips of the 256-thread stride loop
    "sparse3_2x23": _case(S=2, F=23, kind="none", rows=(15, 20, 21)),       # head and wrists, no confidences: 69 entries, less than one block
    "unsorted_rows_1x12": _case(kind="fractional", rows=(20, 4, 15, 1, 7)),
    "blind_sequence_2x6": _case(S=2, F=6, kind="blind"),                    # sequence 1 has c = 0 everywhere
    "frame_dropout_2x6": _case(S=2, F=6, kind="dropout"),                   # ~30 % dead entries (0, negative and NaN confidences), one frame fully dead
    "nan_visible_2x6": _case(S=2, F=6, kind="nan_visible"),                 # a NaN under c = 1 in sequence 1: its term is dropped, as without confidences
    "rot6d_left_leg_1x12": _case(rot="rot6d", kind="left_leg"),
    "tiny_6x2": _case(S=6, F=2, kind="fractional"),                         # F = 2
}
DEAD_FRAME, NAN_AT = 1, (7, 4, 1)      # frame_dropout: frame 1 (of sequence 0) has no live entry; nan_visible: (frame, column, coordinate), frame 7 = frame 1 of sequence 1


@functools.lru_cache(maxsize=None)
def inputs(name):
    """dict of float32 numpy inputs: gt / init [T, 63], joints3d [T, n_obs, 3], conf [T, n_obs] or None, rows (list or None),
    noise [STEPS, T, network inputs]."""
    from dposer_amd.utils.misc import occlude_joints
    c = CASES[name]
    T = c["S"] * c["F"]
    rs = np.random.RandomState(2500 + 100 * c["seed"] + sorted(CASES).index(name))
    f32 = lambda a: np.asarray(a, dtype=np.float32)
    toy = load("g10_normalizer")["toy_pose_samples"]
    gt = f32(toy[rs.choice(len(toy), T, replace=False)])
    init = f32(gt + rs.standard_normal(gt.shape) * 0.05)
    _, jgt = fk_torch.smplx_forward(MC.asset(), torch.tensor(gt, dtype=torch.float64))
    rows = None if c["rows"] is None else list(c["rows"])
    cols = list(range(22)) if rows is None else rows
    n_obs = len(cols)
    joints3d = f32(jgt[:, cols].numpy() + rs.standard_normal((T, n_obs, 3)) * 0.04)
    noise = f32(rs.standard_normal((STEPS, T, 63 if c["rot"] == "axis" else 126)))
    kind = c["kind"]
    conf = None
    if kind in ("ones", "nan_visible"):
        conf = np.ones((T, n_obs), np.float32)
    elif kind == "fractional":
        conf = f32(rs.uniform(0.2, 1.0, (T, n_obs)))
    elif kind == "left_leg":
        j, cf = occlude_joints(torch.tensor(joints3d), part="left_leg")
        joints3d, conf = j.numpy(), cf.numpy()
    elif kind == "blind":
        conf = np.ones((T, n_obs), np.float32)
        conf[c["F"]:] = 0.0
    elif kind == "dropout":
        conf = f32(rs.uniform(0.2, 1.0, (T, n_obs)))
        dead = rs.uniform(size=(T, n_obs)) < 0.3
        dead[DEAD_FRAME] = True
        how = rs.randint(0, 3, size=(T, n_obs))                 # the three ways of not being live: 0, a negative, NaN
        conf[dead] = np.choose(how, [0.0, -0.5, np.nan])[dead].astype(np.float32)
        joints3d[dead] = np.nan
    if kind == "nan_visible":
        joints3d[NAN_AT] = np.nan
    return dict(gt=gt, init=init, joints3d=joints3d, conf=conf, rows=rows, noise=noise)


def _ref(name, dtype, fault, iterations, steps_per_iter, noise, strategy="3"):
    c, x = CASES[name], inputs(name)
    a, b = MC.norm_stats(c["rot"], "zscore")
    return PR.motion_denoise_partial(MC.params(c["rot"]), MC.make_sde("subvp"), MC.asset(), a, b, x["joints3d"], x["gt"], x["init"], noise,
                                     joints_conf=x["conf"], obs_joints=x["rows"], iterations=iterations, steps_per_iter=steps_per_iter, dtype=dtype,
                                     rot6d=c["rot"] == "rot6d", time_strategy=strategy, sample_time=SAMPLE_TIME, frames_per_sequence=c["F"],
                                     fault=fault, details=True)


def run_reference(name, dtype=torch.float64, fault=None):
    """The compared quantities of a case: the whole run (ITERS x SPI steps, time strategy '3') and a run of ONE step at the fixed time of
    strategy '2' (motion_denoise_cases.run_oracle says why), whose gradient is ``grad0`` and whose second moment is ``v0``."""
    z = inputs(name)["noise"]
    out = _ref(name, dtype, fault, ITERS, SPI, z)
    one = _ref(name, dtype, fault, 1, 1, z[:1], strategy="2")
    out["grad0"], out["v0"] = one["grad_steps"][0], one["adam_v"]
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 reference of a case: computed once per process, shared, never written to."""
    out = run_reference(name)
    for v in out.values():
        v.setflags(write=False)
    return out


def distances(got, ref, log_prior_is_total=False):
    """motion_denoise_cases.distances plus the two metrics of the observed / unobserved split; NaN positions must coincide (inf otherwise)."""
    out = MC.distances(got, ref, log_prior_is_total=log_prior_is_total)
    for k in ("MPJPE_observed", "MPJPE_unobserved"):
        a, b = np.asarray(got[k]).reshape(-1), np.asarray(ref[k]).reshape(-1)
        out[k] = 0.0 if np.isnan(a).all() and np.isnan(b).all() else MC._absmax(a, b)
    return out


def worst_ratio(dist):
    """(largest distance / D32 over the quantities, its name)."""
    k = max(dist, key=lambda q: dist[q] / D32[q])
    return dist[k] / D32[k], k
