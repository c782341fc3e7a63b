"""The cases, the float64 references and the comparison band of the one-call SMPLify loop -- shared by tests/test_smplify_ref_cpu.py (which
checks the oracle and measures the band) and tests/test_gpu_smplify.py (which holds the kernels to it).  Test infrastructure: imports
oracle/ and only host-side tables of the package (joint names); no GPU.

Every case is 3 camera + 5 x 3 body iterations on the synthetic SMPL-X asset with sde_N = 500 and time strategy '3', built like golden
g27: ground-truth fits (body poses from g10's toy samples, so the g10 normaliser statistics apply) projected to keypoints plus 2 px of
noise, perturbed initial estimates, recorded prior noise.  All inputs finite, every joint in front of the camera (cam_t z in 18..26).
"""
import functools
import math

import numpy as np
import torch

from helpers import load
from weights import make_weights
from oracle import fk_torch
from oracle import score_ref as R
from oracle import task_loops as TL

NUM_ITERS, SDE_N, STAGES, SEED = 3, 500, 5, 27
N_BODY = NUM_ITERS * STAGES

# ---- the band.  D32: the distance of the float32 oracle from the float64 oracle, the maximum over CASES (measured by
# tests/test_smplify_ref_cpu.py::test_float32_oracle_stays_inside_the_band, which prints every case).  Finals: relative L2; log: the
# largest error of a column relative to the column's largest entry, camera rows and body rows apart (their columns 0 and 3 are
# different quantities).  TOL = 8 x D32: one float32 run is a single sample of rounding noise, and the kernels differ from torch-fp32 by
# the summation orders of the wave butterfly and the sub-mesh, FMA contraction, 1-2 ulp device exp / rsq / division and the bf16x3 pose
# blend.
D32 = {
    "pose": 1.7e-6,          # measured 1.69e-6 (zero_pose_rot6d)
    "betas": 5.0e-7,         # measured 4.93e-7 (rot6d_zscore: the 250x gain of its std = 3.9e-3 table)
    "cam_t": 5.3e-8,         # measured 5.27e-8 (axis_minmax): half an ulp of t_z ~ 22
    "reprojection": 2.8e-6,  # measured 2.75e-6 (rot6d_none)
    "log_cam_0": 8.7e-7,     # measured 8.69e-7 (conf_edges)
    "log_cam_3": 1.7e-4,     # measured 1.67e-4 (rot6d_zscore): the depth term squares t_z - t_z_est ~ 0.03, a difference of two numbers ~ 22
    "log_body_0": 5.6e-7,    # measured 5.58e-7 (rot6d_none)
    "log_body_1": 1.7e-7,    # measured 1.66e-7 (axis_zscore)
    "log_body_2": 1.6e-7,    # measured 1.56e-7 (zero_pose_rot6d)
    "log_body_3": 1.0e-6,    # measured 9.92e-7 (zero_pose_rot6d)
}
TOL_FACTOR = 8.0
TOL = {k: TOL_FACTOR * v for k, v in D32.items()}


def joint_tables():
    """The 49-row joint map of body_model/smpl.py and the keypoint indices of the camera loss / the ignored joints."""
    from dposer_amd.body_model import constants
    jmap = [constants.JOINT_MAP[n] for n in constants.JOINT_NAMES]
    jmap[:25] = constants.SMPLX_OPENPOSE_25
    ids = lambda names: [constants.JOINT_IDS[n] for n in names]
    return jmap, dict(op_joints=ids(["OP RHip", "OP LHip", "OP RShoulder", "OP LShoulder"]),
                      gt_joints=ids(["Right Hip", "Left Hip", "Right Shoulder", "Left Shoulder"]),
                      ign_joints=ids(["OP Neck", "OP RHip", "OP LHip", "Right Hip", "Left Hip"]))


@functools.lru_cache(maxsize=None)
def assets():
    from dposer_amd.body_model.synthetic import make_synthetic_smplx_asset
    full = make_synthetic_smplx_asset(seed=0)
    jmap, _ = joint_tables()
    return full, TL.smplify_asset_subset(full, jmap)


def t_list():
    """run/smplify.py:160-162 (time strategy '3': an int64 tensor times a python float is fp32 arithmetic) through
    ``timesteps = linspace(T, 1e-3, N)`` (:33)."""
    ts = torch.linspace(1.0, 1e-3, SDE_N)
    quan = [SDE_N - math.floor(float(np.float32(N_BODY - i - 1) * np.float32(SDE_N / (20.0 * N_BODY)))) - 5 for i in range(N_BODY)]
    return [float(ts[q]) for q in quan]


def norm_stats(rot, norm):
    g = load("g10_normalizer")
    if norm == "none":
        return None, None
    a, b = ("mean_poses", "std_poses") if norm == "zscore" else ("min_poses", "max_poses")
    n = 2 if norm == "zscore" else 1
    return g[f"stats/{rot}_normalize{n}/{a}"], g[f"stats/{rot}_normalize{n}/{b}"]


# name -> (B, rot, norm, sde kind, what is special)
CASES = {
    "axis_none": (3, "axis", "none", "subvp", "g27"), "axis_zscore": (3, "axis", "zscore", "subvp", "g27"),
    "axis_minmax": (3, "axis", "minmax", "subvp", "g27"), "rot6d_none": (3, "rot6d", "none", "subvp", "g27"),
    "rot6d_zscore": (3, "rot6d", "zscore", "subvp", "g27"), "rot6d_minmax": (3, "rot6d", "minmax", "subvp", "g27"),
    "conf_edges": (5, "axis", "zscore", "subvp", "conf"),
    "zero_pose_axis": (3, "axis", "zscore", "subvp", "zero"), "zero_pose_rot6d": (3, "rot6d", "zscore", "subvp", "zero"),
    "b1_scalar_focal": (1, "axis", "zscore", "subvp", "scalar"),
    "vp_discrete": (3, "axis", "zscore", "vp_discrete", "g27"), "ve": (3, "axis", "zscore", "ve", "g27"), "vp": (3, "axis", "zscore", "vp", "g27"),
}


def make_sde(kind):
    return {"subvp": lambda: R.SubVP(N=SDE_N), "vp": lambda: R.VP(N=SDE_N), "vp_discrete": lambda: R.VP(N=SDE_N, discrete=True),
            "ve": lambda: R.VE(N=SDE_N)}[kind]()


@functools.lru_cache(maxsize=None)
def inputs(name):
    """dict of float32 numpy inputs (focal_length: [B], or a python float for the scalar case)."""
    B, rot, _, _, special = CASES[name]
    jmap, tab = joint_tables()
    rs = np.random.RandomState(2800 + sorted(CASES).index(name))
    f32 = lambda a: np.asarray(a, dtype=np.float32)
    toy = load("g10_normalizer")["toy_pose_samples"]
    gt_pose = f32(np.concatenate([rs.standard_normal((B, 3)) * 0.2, toy[rs.choice(len(toy), B, replace=False)]], axis=1))
    gt_betas = f32(rs.standard_normal((B, 10)) * 0.5)
    gt_t = f32(np.stack([rs.uniform(-0.2, 0.2, B), rs.uniform(-0.2, 0.2, B), rs.uniform(18, 23, B)], 1))
    focal = 5000.0 if special == "scalar" else f32(rs.uniform(4000, 6000, B))
    center = f32(112 + rs.uniform(-8, 8, (B, 2)))
    d = lambda a: torch.tensor(a, dtype=torch.float64)
    _, j = fk_torch.smplx_forward(assets()[1], d(gt_pose[:, 3:]), betas=d(gt_betas), global_orient=d(gt_pose[:, :3]), transl=d(gt_t))
    proj = TL.smplify_project(j[:, jmap], focal if special == "scalar" else d(focal), d(center)).numpy()
    kp = f32(np.concatenate([proj + rs.standard_normal((B, 49, 2)) * 2.0, rs.uniform(0.3, 1.0, (B, 49, 1))], axis=2))
    if special == "conf":
        kp[0, :, 2] = 0.0                              # no confident keypoint: only the priors move this image's body stage
        kp[3, tab["op_joints"][3], 2] = -0.5           # a negative OP confidence: GT branch in the camera stage, weight 0.25 in the body stage
    else:
        if B > 1:
            kp[1, tab["op_joints"][0], 2] = 0.0        # image 1: OP RHip missing, the camera loss falls back to the GT joints
        if B > 2:
            kp[2, rs.choice(49, 8, replace=False), 2] = 0.0
    init_pose = f32(gt_pose + rs.standard_normal(gt_pose.shape) * 0.1)
    if special == "zero":
        init_pose[:, 3:] = 0.0                         # the usual start of a real fit: Rodrigues' + 1e-8 direction
    init_betas = f32(gt_betas * 0.5 + rs.standard_normal(gt_betas.shape) * 0.1)
    init_cam_t = f32(gt_t * np.array([1.0, 1.0, 1.1]) + rs.standard_normal(gt_t.shape) * 0.02)
    assert 18.0 < init_cam_t[:, 2].min() and init_cam_t[:, 2].max() < 26.0
    noise = f32(rs.standard_normal((N_BODY, B, 63 if rot == "axis" else 126)))
    return dict(init_pose=init_pose, init_betas=init_betas, init_cam_t=init_cam_t, camera_center=center, keypoints=kp, focal_length=focal,
                noise=noise)


def params(rot):
    p = dict(make_weights(SEED, D=63 if rot == "axis" else 126))
    p["sigmas"] = R.sigma_table()
    return p


def run_oracle(name, dtype=torch.float64, fault=None, noise=None):
    B, rot, norm, kind, _ = CASES[name]
    x = inputs(name)
    jmap, tab = joint_tables()
    a, b = norm_stats(rot, norm)
    return TL.smplify_optimize(params(rot), make_sde(kind), assets()[1], jmap, x["init_pose"], x["init_betas"], x["init_cam_t"],
                               x["camera_center"], x["keypoints"], t_list(), x["noise"] if noise is None else noise,
                               focal_length=x["focal_length"], num_iters=NUM_ITERS, rot6d=rot == "rot6d", norm_mode=norm, norm_a=a, norm_b=b,
                               dtype=dtype, fault=fault, **tab)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 oracle of a case: computed once per process, shared, never written to."""
    out = run_oracle(name)
    for v in out.values():
        v.setflags(write=False)
    return out


def distances(got, ref):
    """The compared quantities of one run against a reference, in the units of D32 / TOL."""
    f = lambda a: np.asarray(a, dtype=np.float64)
    out = {}
    for k in ("pose", "betas", "cam_t", "reprojection"):
        out[k] = float(np.linalg.norm(f(got[k]) - f(ref[k])) / max(np.linalg.norm(f(ref[k])), 1e-30))
    gl, rl = f(got["log"]), f(ref["log"])
    assert gl.shape == rl.shape
    for tag, rows, cols in (("cam", slice(0, NUM_ITERS), (0, 3)), ("body", slice(NUM_ITERS, None), (0, 1, 2, 3))):
        for c in cols:
            out[f"log_{tag}_{c}"] = float(np.abs(gl[rows, :, c] - rl[rows, :, c]).max() / np.abs(rl[rows, :, c]).max())
    return out


def worst_ratio(dist):
    """(largest distance / D32 over the quantities, its name)."""
    k = max(dist, key=lambda q: dist[q] / D32[q])
    return dist[k] / D32[k], k
