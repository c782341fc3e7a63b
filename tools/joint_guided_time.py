"""ms per loop index of dposer_joint_guided_sampler vs dposer_guided_sampler (DPS) at B = 500 and 16384, interleaved:
prints the rows of profiles/joint_guided_time.md (median / min / max ms per loop index of an N = 100 run)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import numpy as np
import torch
import test_gpu_joint_guided as T
from dposer_amd.algorithms.advanced import sampling
from dposer_amd.body_model.body_model import BodyModel
import rot_ref as rr
dev = T.DEV
bm = BodyModel(rr.body_asset(), num_betas=10, num_expressions=0, model_type="smplx").to(dev)
out = []
N = 100
for prec in ("bf16", "fp32"):
    cfg, m, p = T._model(33, prec)
    m.freeze_packed = True
    m._engine().packed(m.flat_params(), with_backward=True, force=True)
    for B in (500, 16384):
        q = T._sampler_inputs(B, 5, 1, n_obs=22, conf_kind="zeros")
        sde = T._sde("subvp", N)
        ts = torch.linspace(sde.T, 1e-3, N)
        x0 = T._dev(q["x0"]); obs = T._dev(q["obs"]); conf = T._dev(q["conf"]); root = T._dev(q["root"]); tr = T._dev(q["transl"])
        nz = T._normalizer("zscore")
        pobs = T._dev(np.random.RandomState(1).standard_normal((B, 63)) * 0.5); mask = torch.ones(B, 63, device=dev); mask[:, :12] = 0

        def joint(scope):
            return sampling.fused_joint_guided_sample(m, sde, x0, ts, bm, nz, obs, joints_conf=conf, root_orient=root, trans=tr, norm=scope, grad_step=0.7, seed=3)

        def dps():
            return sampling.fused_guided_sample(m, sde, x0, ts, pobs, mask, method="dps", grad_step=0.7, seed=3)

        runs = {"joints, sample scope": lambda: joint("sample"), "joints, batch scope": lambda: joint("batch"), "pose mask (DPS)": dps}
        for f in runs.values():
            f(); f()
        ms = {k: [] for k in runs}
        for _ in range(5):
            for k, f in runs.items():
                torch.cuda.synchronize(); t0 = time.perf_counter()
                f()
                torch.cuda.synchronize(); ms[k].append((time.perf_counter() - t0) / N * 1e3)
        for k in runs:
            out.append(f"| {prec} | {B} | {k} | {np.median(ms[k]):.4f} | {min(ms[k]):.4f} | {max(ms[k]):.4f} |")
            print(out[-1], flush=True)
