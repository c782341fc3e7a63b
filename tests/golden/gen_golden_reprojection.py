#!/usr/bin/env python3
"""Golden g34_reprojection: the reference's own body_fitting_loss(..., pose_prior=None, output='reprojection')
(lib/body_model/fitting_losses.py:59-101: perspective_projection, gmof, joints_conf ** 2), captured by importing the reference
(read-only) -- run in the build container only:

    python tests/golden/gen_golden_reprojection.py

Random model_joints [4, 22, 3] per focal length (5000 and 1000): depths in 2..6 m, back-projected from points inside a 1000 x 800 image;
keypoints = their projection + an offset of 40..120 px in a random direction (a few outliers of hundreds of pixels more, so that gmof
bends); confidences in 0.2..1.5 with some exact zeros; sigma 100.  Stored: the inputs and the [4, 22] output per focal length, nothing else.

Why the offsets are no smaller.  The reference computes in float32 and adds the centre to the projection before it takes the keypoint off:
with image coordinates up to 1000 px its residual carries an absolute error of up to ~1.1e-4 px (X / Z: 3e-5 at 500 px; focal * (X / Z):
1.5e-5; + centre: 3e-5; - keypoint: 3e-5), so a term rho(ru) + rho(rv) carries up to 2 sqrt(2) 1.1e-4 / |r| relative: 7.8e-6 at |r| = 40 px.
The CPU test holds the float64 rule to this golden at 1e-5 relative, which is therefore the reference's own rounding on these inputs.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from gen_golden import save  # noqa: E402  (puts the reference on sys.path and stubs what it imports at module scope)


def main():
    import lib.body_model.fitting_losses as ref_fl
    rs = np.random.RandomState(34)
    B, n, sigma = 4, 22, 100.0
    focals = np.array([5000.0, 1000.0], dtype=np.float32)
    center = (np.array([500.0, 400.0]) + rs.uniform(-20, 20, (B, 2))).astype(np.float32)
    conf = rs.uniform(0.2, 1.5, (B, n)).astype(np.float32)
    conf[rs.uniform(size=(B, n)) < 0.25] = 0.0
    cam_t = rs.standard_normal((B, 3)).astype(np.float32)                    # handed over and, as the reference has it, never added
    jts, kps, outs = [], [], []
    for f in focals:
        Z = rs.uniform(2.0, 6.0, (B, n, 1))
        uv = rs.uniform([100.0, 100.0], [900.0, 700.0], (B, n, 2))
        joints = np.concatenate([(uv - center[:, None, :]) / f * Z, Z], axis=2).astype(np.float32)
        proj = f * joints[..., :2] / joints[..., 2:3] + center[:, None, :]
        ang = rs.uniform(0, 2 * np.pi, (B, n))
        off = rs.uniform(40.0, 120.0, (B, n, 1)) * np.stack([np.cos(ang), np.sin(ang)], axis=2)
        far = rs.uniform(size=(B, n)) < 0.15
        off[far] += rs.choice([-1.0, 1.0], size=(int(far.sum()), 2)) * rs.uniform(150, 600, (int(far.sum()), 2))
        kp = (proj + off).astype(np.float32)
        out = ref_fl.body_fitting_loss(torch.zeros(B, 69), torch.zeros(B, 10), torch.tensor(joints), torch.tensor(cam_t), torch.tensor(center),
                                       torch.tensor(kp), torch.tensor(conf), None, None, focal_length=float(f), sigma=sigma, output="reprojection",
                                       verbose=False)
        assert tuple(out.shape) == (B, n)
        jts.append(joints)
        kps.append(kp)
        outs.append(out.numpy())
    save("g34_reprojection", model_joints=np.stack(jts), camera_center=center, camera_t=cam_t, joints_conf=conf, focal=focals, sigma=np.float32(sigma),
         keypoints=np.stack(kps), reprojection=np.stack(outs))


if __name__ == "__main__":
    main()
