"""fk_joints forward + backward, grad="chain" vs grad="lbs", interleaved in one process: prints the rows of profiles/fk_joints_backward_time.md
(median / min / max ms of a forward + backward, peak bytes per pose beyond the live inputs)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from dposer_amd.body_model.body_model import BodyModel
from dposer_amd.body_model.synthetic import make_synthetic_smplx_asset
dev = "cuda:0"
bm = BodyModel(make_synthetic_smplx_asset(seed=0)).to(dev)
out = []
for B in (4096, 65536):
    rs = np.random.RandomState(B)
    p = torch.tensor((rs.standard_normal((B, 63)) * 0.3).astype(np.float32), device=dev, requires_grad=True)
    r = torch.tensor((rs.standard_normal((B, 3)) * 0.3).astype(np.float32), device=dev, requires_grad=True)
    w = torch.tensor(rs.standard_normal((B, 22, 3)).astype(np.float32), device=dev)

    def step(route):
        p.grad = r.grad = None
        (bm.fk_joints(p, root_orient=r, grad=route) * w).sum().backward()

    grads = {}
    for route in ("chain", "lbs"):
        for _ in range(3):
            step(route)
        grads[route] = (p.grad.clone(), r.grad.clone())
    rel = float((grads["chain"][0] - grads["lbs"][0]).norm() / grads["lbs"][0].norm())
    reps, rounds = (200, 7) if B == 4096 else (20, 7)
    ms = {"chain": [], "lbs": []}
    for _ in range(rounds):
        for route in ("chain", "lbs"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                step(route)
            torch.cuda.synchronize()
            ms[route].append((time.perf_counter() - t0) / reps * 1e3)
    peak = {}
    for route in ("chain", "lbs"):
        p.grad = r.grad = None
        torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        step(route)
        torch.cuda.synchronize()
        peak[route] = (torch.cuda.max_memory_allocated() - base) / B
    for route in ("chain", "lbs"):
        out.append(f"| {B} | {route} | {np.median(ms[route]):.4f} | {min(ms[route]):.4f} | {max(ms[route]):.4f} | {peak[route]:.0f} |")
    out.append(f"| {B} | lbs / chain | {np.median(ms['lbs']) / np.median(ms['chain']):.1f}x | | | {peak['lbs'] / peak['chain']:.0f}x | pose-gradient rel-L2 chain vs lbs {rel:.1e}")
    print("\n".join(out[-3:]), flush=True)
