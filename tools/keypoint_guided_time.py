"""ms per loop index of dposer_keypoint_guided_sampler vs dposer_joint_guided_sampler at B = 500 and 16384, interleaved:
prints the rows of profiles/keypoint_guided_time.md (median / min / max ms per loop index of an N = 100 run)."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)
import rot_ref as rr  # noqa: E402
from gpu_common import DEV, make_model  # noqa: E402
from dposer_amd.algorithms.advanced import sampling, sde_lib  # noqa: E402
from dposer_amd.body_model.body_model import BodyModel  # noqa: E402
from dposer_amd.dataset.AMASS import Posenormalizer  # noqa: E402

N, FOCAL, ROUNDS = 100, 5000.0, 5


def dev(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device=DEV)


def problem(bm, nz, B, seed):
    """The same body observed twice: its 22 joints in 3D (+ 5 cm noise) and their projection (+ 10 px noise); 30 % dead entries."""
    rs = np.random.RandomState(seed)
    root = dev(rs.standard_normal((B, 3)) * 0.3)
    cam = dev(np.concatenate([rs.standard_normal((B, 2)) * 0.2, rs.uniform(3.0, 5.0, (B, 1))], axis=1))
    center = dev(np.tile([500.0, 400.0], (B, 1)))
    with torch.no_grad():
        J = bm.fk_joints(nz.offline_denormalize(dev(rs.standard_normal((B, 63)) * 0.5)), root_orient=root, trans=cam)[:, :22]
    obs = J + dev(rs.standard_normal((B, 22, 3)) * 0.05)
    kp = FOCAL * J[..., :2] / J[..., 2:3] + center[:, None] + dev(rs.standard_normal((B, 22, 2)) * 10.0)
    conf = rs.uniform(0.2, 1.5, (B, 22))
    conf[rs.uniform(size=(B, 22)) < 0.3] = 0.0
    return dict(x0=dev(rs.standard_normal((B, 63))), root=root, cam=cam, center=center, focal=dev(np.full(B, FOCAL)), obs=obs, kp=kp, conf=dev(conf))


def main():
    bm = BodyModel(rr.body_asset(), num_betas=10, num_expressions=0, model_type="smplx").to(DEV)
    rs = np.random.RandomState(4)
    stats = dict(mean_poses=torch.tensor(rs.standard_normal(63) * 0.1, dtype=torch.float32),
                 std_poses=torch.tensor(rs.uniform(0.2, 0.5, 63), dtype=torch.float32),
                 min_poses=torch.full((63,), -2.0), max_poses=torch.full((63,), 2.0))
    nz = Posenormalizer(stats, device=DEV, normalize=True, min_max=False, rot_rep="axis")
    sde = sde_lib.subVPSDE(0.1, 20.0, N)
    ts = torch.linspace(sde.T, 1e-3, N)
    for prec in ("bf16", "fp32"):
        _, m, _ = make_model(33, precision=prec)
        m.freeze_packed = True
        m._engine().packed(m.flat_params(), with_backward=True, force=True)
        for B in (500, 16384):
            q = problem(bm, nz, B, 5)

            def joints(scope):
                return sampling.fused_joint_guided_sample(m, sde, q["x0"], ts, bm, nz, q["obs"], joints_conf=q["conf"], root_orient=q["root"],
                                                          trans=q["cam"], norm=scope, grad_step=0.7, seed=3)

            def keypoints(scope):
                return sampling.fused_keypoint_guided_sample(m, sde, q["x0"], ts, bm, nz, q["kp"], keypoints_conf=q["conf"], cam_t=q["cam"],
                                                             camera_center=q["center"], focal=q["focal"], sigma=100.0, z_near=0.1,
                                                             root_orient=q["root"], norm=scope, grad_step=0.7 * 4.0 / FOCAL, seed=3)

            legs = {"keypoints, sample scope": lambda: keypoints("sample"), "joints, sample scope": lambda: joints("sample"),
                    "keypoints, batch scope": lambda: keypoints("batch"), "joints, batch scope": lambda: joints("batch")}
            for run in legs.values():                # two warm-up runs per leg
                run()
                run()
            ms = {name: [] for name in legs}
            for _ in range(ROUNDS):
                for name, run in legs.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    run()
                    torch.cuda.synchronize()
                    ms[name].append((time.perf_counter() - t0) / N * 1e3)
            for name in legs:
                print(f"| {prec} | {B} | {name} | {np.median(ms[name]):.4f} | {min(ms[name]):.4f} | {max(ms[name]):.4f} |", flush=True)


if __name__ == "__main__":
    main()
