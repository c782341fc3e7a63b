"""The cases, the float64 references and the comparison band of the one-call motion-denoising loop -- shared by
tests/test_motion_denoise_ref_cpu.py (which checks the oracle and measures the band) and tests/test_gpu_motion_denoise.py (which holds
the kernels to it).  Test infrastructure: imports oracle/ and the synthetic asset; no GPU.

Every case is at most 2 outer iterations of 3 Adam steps on the synthetic SMPL-X asset with sde_N = 500, built from a seed like
tests/test_gpu_tasks.py::_md_setup: distinct toy poses of g10 as the ground truth (so the g10 normaliser statistics apply), initial poses =
ground truth + 0.05 noise, observed joints = the ground truth's joints + 0.04 noise, recorded prior noise.  No case has an exactly zero
joint residual or two identical frames: there the kernels clamp on purpose and the reference yields NaN (csrc/tasks.hip).
"""
import functools

import numpy as np
import torch

from helpers import load
from weights import make_weights
from oracle import fk_torch
from oracle import score_ref as R
from oracle import task_loops as TL

ITERS, SPI, SDE_N, SEED = 2, 3, 500, 63
STEPS = ITERS * SPI
BETA1, BETA2 = 0.9, 0.999

# ---- the band.  D32: the distance of the float32 oracle from the float64 oracle, the maximum over CASES -- MEASURED by
# tests/test_motion_denoise_ref_cpu.py::test_float32_oracle_stays_inside_the_band, which prints every case and asserts that a fresh
# measurement stays within 2 x of these constants.  A float32 run is one sample of rounding noise and another host's BLAS / libm draws
# another (the same case moved by up to 2 x between two hosts): each constant is the larger of the two hosts' maxima, both recorded.  pose (after every step) and the metrics (cm): largest absolute difference; grad0 /
# v0 (the first step's gradient and second moment, from a one-step run), adam_m / adam_v (after the last step): largest difference
# relative to the largest magnitude in the tensor; log_c: the largest error of a loss-log column relative to the column's largest entry.
# TOL = 8 x D32, the factor of tests/smplify_cases.py (one float32 run is a single sample of rounding noise; the kernels differ from
# torch-fp32 by summation orders, FMA contraction and 1-2 ulp device functions).
D32 = {
    "pose": 1.9e-6,          # measured 1.80e-6 / 1.88e-6 (nan_observation on both hosts)
    "grad0": 1.1e-6,         # measured 1.01e-6 (vp) / 1.10e-6 (large_angle_rot6d)
    "v0": 1.6e-6,            # measured 1.56e-6 / 1.56e-6 (large_angle_rot6d)
    "adam_m": 2.4e-6,        # measured 1.24e-6 (rot6d_zscore) / 2.43e-6 (axis_minmax)
    "adam_v": 2.1e-6,        # measured 1.25e-6 / 2.11e-6 (axis_none)
    "log_0": 1.6e-7,         # measured 1.49e-7 (seq_6x2) / 1.59e-7 (seq_2x23)
    "log_1": 1.7e-7,         # measured 1.49e-7 (axis_zscore) / 1.67e-7 (seq_6x2)
    "log_2": 2.8e-7,         # measured 2.77e-7 (betas_per_frame) / 2.28e-7 (weighted)
    "init_MPJPE": 1.4e-6,    # measured 1.37e-6 (axis_zscore) / 1.42e-6 (fourier), cm
    "MPJPE": 1.8e-6,         # measured 1.10e-6 (vp_discrete) / 1.77e-6 (fourier), cm
    "MPVPE": 8.7e-6,         # measured 8.68e-6 (seq_3x8) / 8.35e-6 (fourier), cm: the mean over 10475 vertex distances of ~10 cm
}
TOL_FACTOR = 8.0
TOL = {k: TOL_FACTOR * v for k, v in D32.items()}
# the condition on the inputs: Adam turns a near-zero gradient coordinate into a coin flip of 2 lr, so the seeds are chosen such that the
# float32 oracle's pose stays within 1e-5 (the tolerance of tests/test_gpu_tasks.py::test_motion_denoise_steps_match_oracle) of the
# float64 oracle's after every step, with every coordinate compared
POSE_D32_MAX = 1e-5


def _case(S=1, F=12, rot="axis", norm="zscore", kind="subvp", emb="positional", weighted=False, strategy="3", betas=False, special=None,
          seed=0):
    return dict(S=S, F=F, rot=rot, norm=norm, kind=kind, emb=emb, weighted=weighted, strategy=strategy, betas=betas, special=special, seed=seed)


SAMPLE_TIME = 300      # time strategy '2'
CASES = {
    "axis_none": _case(norm="none"), "axis_zscore": _case(), "axis_minmax": _case(norm="minmax"),
    "rot6d_zscore": _case(rot="rot6d"), "rot6d_minmax": _case(rot="rot6d", norm="minmax"),
    "fourier": _case(emb="fourier"),
    "vp": _case(kind="vp"), "vp_discrete": _case(kind="vp_discrete"), "ve": _case(kind="ve"), "ve_discrete": _case(kind="ve_discrete"),
    "weighted": _case(weighted=True, strategy="2"),      # (a fixed mid-range t: at the t = 3e-3 the last step of strategy '3' draws, the weight sqrt(1 + snr) makes float32 itself 5 x noisier)
    "strategy2": _case(strategy="2"),
    "betas_per_frame": _case(S=2, F=6, betas=True),
    "seq_3x8": _case(S=3, F=8),
    "seq_2x23": _case(S=2, F=23),          # a workgroup of four poses straddles the sequence boundary
    "seq_6x2": _case(S=6, F=2),            # every frame has exactly one neighbour
    "zero_pose_rot6d": _case(rot="rot6d", special="zero"),        # one frame starts at the zero pose: Rodrigues' + 1e-8 direction
    "large_angle_rot6d": _case(rot="rot6d", special="large"),     # one joint of one frame rotated by more than 3 rad
    "nan_observation": _case(S=2, F=6, special="nan"),            # sequence 1 observes a NaN: its data term is dropped, sequence 0 is untouched
}
ZERO_FRAME, LARGE_FRAME, LARGE_JOINT, NAN_AT = 2, 5, 3, (7, 4, 1)      # (frame, joint, coordinate) of the NaN: frame 7 = frame 1 of sequence 1


def make_sde(kind):
    return {"subvp": lambda: R.SubVP(N=SDE_N), "vp": lambda: R.VP(N=SDE_N), "vp_discrete": lambda: R.VP(N=SDE_N, discrete=True),
            "ve": lambda: R.VE(N=SDE_N), "ve_discrete": lambda: R.VE(N=SDE_N, discrete=True)}[kind]()


@functools.lru_cache(maxsize=None)
def asset():
    from dposer_amd.body_model.synthetic import make_synthetic_smplx_asset
    return make_synthetic_smplx_asset(seed=0)


@functools.lru_cache(maxsize=None)
def rot6d_stats():
    """126-D statistics of g10's poses in the 6-D representation, built as tests/test_gpu_tasks.py builds them for its rot6d test."""
    raw = torch.tensor(load("g10_normalizer")["raw"], dtype=torch.float64)
    six = fk_torch.batch_rodrigues(raw.reshape(-1, 3))[:, :, :2].reshape(raw.shape[0], -1).numpy()
    f32 = lambda a: np.asarray(a, dtype=np.float32)
    return dict(mean_poses=f32(six.mean(0)), std_poses=f32(six.std(0) + 1e-3), min_poses=f32(six.min(0) - 1e-3), max_poses=f32(six.max(0) + 1e-3))


def stats(rot):
    """The four statistics tensors of a Posenormalizer, as float32 numpy."""
    if rot == "rot6d":
        return rot6d_stats()
    g = load("g10_normalizer")
    return {k.split("/")[-1]: g[k] for k in g.files if k.startswith("stats/axis_normalize")}


def norm_stats(rot, norm):
    st = stats(rot)
    if norm == "none":
        return None, None
    return (st["mean_poses"], st["std_poses"]) if norm == "zscore" else (st["min_poses"], st["max_poses"])


@functools.lru_cache(maxsize=None)
def inputs(name):
    """dict of float32 numpy inputs: gt / init [T, 63], joints3d [T, 22, 3], noise [STEPS, T, network inputs], betas [T, 10] or None."""
    c = CASES[name]
    T = c["S"] * c["F"]
    rs = np.random.RandomState(1500 + 100 * c["seed"] + sorted(CASES).index(name))
    f32 = lambda a: np.asarray(a, dtype=np.float32)
    toy = load("g10_normalizer")["toy_pose_samples"]
    gt = f32(toy[rs.choice(len(toy), T, replace=False)])
    init = f32(gt + rs.standard_normal(gt.shape) * 0.05)
    betas = f32(rs.standard_normal((T, 10)) * 0.5) if c["betas"] else None
    if c["special"] == "zero":
        init[ZERO_FRAME] = 0.0
    if c["special"] == "large":
        axis = rs.standard_normal(3)
        init[LARGE_FRAME, 3 * LARGE_JOINT:3 * LARGE_JOINT + 3] = f32(3.05 * axis / np.linalg.norm(axis))
    d = lambda a: None if a is None else torch.tensor(a, dtype=torch.float64)
    _, jgt = fk_torch.smplx_forward(asset(), d(gt), betas=d(betas))
    joints3d = f32(jgt[:, :22].numpy() + rs.standard_normal((T, 22, 3)) * 0.04)
    if c["special"] == "nan":
        joints3d[NAN_AT] = np.nan
    noise = f32(rs.standard_normal((STEPS, T, 63 if c["rot"] == "axis" else 126)))
    return dict(gt=gt, init=init, joints3d=joints3d, noise=noise, betas=betas)


def params(rot, emb="positional"):
    p = dict(make_weights(SEED, D=63 if rot == "axis" else 126, fourier=emb == "fourier"))
    p["sigmas"] = R.sigma_table()
    return p


def _oracle(name, dtype, fault, iterations, steps_per_iter, noise, strategy=None):
    c, x = CASES[name], inputs(name)
    a, b = norm_stats(c["rot"], c["norm"])
    return TL.motion_denoise_optimize(params(c["rot"], c["emb"]), make_sde(c["kind"]), asset(), a, b, x["joints3d"], x["gt"], x["init"], noise,
                                      iterations=iterations, steps_per_iter=steps_per_iter, dtype=dtype, norm_mode=c["norm"],
                                      rot6d=c["rot"] == "rot6d", embedding_type=c["emb"], weighted=c["weighted"],
                                      time_strategy=strategy or c["strategy"],
                                      sample_time=SAMPLE_TIME, betas=x["betas"], frames_per_sequence=c["F"], fault=fault, details=True)


def run_oracle(name, dtype=torch.float64, fault=None, noise=None):
    """The compared quantities of a case from the oracle: the whole run (ITERS x SPI steps) and a run of ONE step, whose gradient is
    ``grad0`` and whose second moment is ``v0`` = (1 - beta2) grad0^2.  The one-step run is at the fixed time of strategy '2' in every
    case: a one-step call under strategy '3' draws t = 3e-3, where x0_hat = x0 to 1e-3 and the prior term all but vanishes from the
    gradient -- a wrongly scaled prior gradient would pass (measured: a missing factor 2 of min-max moved grad0 by 2 x its tolerance
    there, by 1e4 x at t = 0.4)."""
    z = inputs(name)["noise"] if noise is None else noise
    out = _oracle(name, dtype, fault, ITERS, SPI, z)
    one = _oracle(name, dtype, fault, 1, 1, z[:1], strategy="2")
    out["grad0"], out["v0"] = one["grad_steps"][0], one["adam_v"]
    assert np.allclose(one["adam_m"], (1 - BETA1) * out["grad0"], rtol=1e-5, atol=0, equal_nan=True)
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 oracle of a case: computed once per process, shared, never written to."""
    out = run_oracle(name)
    for v in out.values():
        v.setflags(write=False)
    return out


def _absmax(a, b):
    """Largest |a - b|; a NaN must sit where the reference has one (inf otherwise) and is then left out."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    na, nb = np.isnan(a), np.isnan(b)
    if not np.array_equal(na, nb):
        return float("inf")
    return float(np.abs(a - b)[~nb].max())


def distances(got, ref, log_prior_is_total=False):
    """The compared quantities of one run against a reference, in the units of D32 / TOL.  ``got['pose_steps']``, where present, is
    compared step by step (the float32 oracle); else the final pose.  ``log_prior_is_total``: column 2 of ``got['log']`` holds the batch
    total in every sequence's row (the one-call loop's layout, include/dposer_hip.h) and is compared with the sum of the reference's
    per-sequence prior terms."""
    out = {"pose": _absmax(got["pose_steps"], ref["pose_steps"]) if "pose_steps" in got else _absmax(got["pose"], ref["pose"])}
    for k in ("grad0", "v0", "adam_m", "adam_v"):
        if k in got and k in ref:          # (a run without the one-step call has no grad0 / v0)
            out[k] = _absmax(got[k], ref[k]) / float(np.abs(ref[k]).max())
    gl, rl = np.asarray(got["log"], dtype=np.float64), np.asarray(ref["log"], dtype=np.float64)
    assert gl.shape == rl.shape, (gl.shape, rl.shape)
    for c in (0, 1, 2):
        want = rl[:, :, c]
        if c == 2 and log_prior_is_total:
            want = np.repeat(want.sum(axis=1, keepdims=True), rl.shape[1], axis=1)
        out[f"log_{c}"] = _absmax(gl[:, :, c], want) / float(np.abs(want).max())
    for k in ("init_MPJPE", "MPJPE", "MPVPE"):
        out[k] = _absmax(np.asarray(got[k]).reshape(-1), np.asarray(ref[k]).reshape(-1))
    return out


def worst_ratio(dist):
    """(largest distance / D32 over the quantities, its name)."""
    k = max(dist, key=lambda q: dist[q] / D32[q])
    return dist[k] / D32[k], k
