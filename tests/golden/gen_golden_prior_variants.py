#!/usr/bin/env python3
"""Golden g31_prior_variants: the reference's own multi-step (DDIM) prior losses and RED-Diff regulariser -- captured by importing the
reference (read-only); run in the build container only:

    python tests/golden/gen_golden_prior_variants.py

The reference's UNBOUND methods run on a small stand-in object that carries what they read (sde, score_fn, rsde, loss_fn, batch_size):
  run.completion.DPoserComp.loss(multi_denoise=True)            weighted and not          (completion.py:112-149, N = 10, torch.mean)
  run.smplify.DPoser.DPoser_loss(multi_denoise=True)                                      (smplify.py:76-107, N = 5, sum / batch_size)
  run.motion_denoising.MotionDenoise.DPoser_loss(multi_denoise=True)                      (motion_denoising.py:106-143, N = 10, sum / batch_size)
  run.motion_denoising.MotionDenoise.RED_Diff                                             (motion_denoising.py:145-154)
  multi_step_denoise directly, N in {1, 5, 10}, and one_step_denoise for comparison
on the CPU, B = 16, D = 63, the recorded randn draw as z, autograd's gradient w.r.t. x_0.
Cases: sub-VP and VP at t in {0.3, 0.5}, VE at t = 0.7; RED-Diff additionally at t = 0.1 (sub-VP, VP) and t = 0.3 (VE).

Per stored case the generator ASSERTS (and stores the measured values):
  1. rel. L2 distance between the N-step (N = 5, 10) and the one-step estimate >= 5 x the loosest tolerance the case is tested at
     (sub-VP / VP: TOL_BF16; VE, tested in fp32 / bf16x3 only: TOL_FP32) -- a port that returned the one-step estimate cannot pass;
  2. ||x0 - est|| / ||est|| >= 0.5 -- the bound of the multi-step gradient and loss is the estimate's bound divided by it;
  3. for every RED-Diff case whose scalar is compared (`red_*_scalar_ok`): the float64 scalar moves by <= 2 x the relative perturbation
     when the score is perturbed by 1e-3 (uniformly, and with random signs).  Where signed terms cancel (sub-VP / VP at t = 0.5) the
     scalar is stored but flagged as not compared.
If a draw fails a condition, change the seed, not the bound.
"""
import os
import sys
import types

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
import gen_golden as G  # noqa: E402
from gen_golden import Recorder, build_model, ref_completion, ref_mutils, ref_sde, save, toy_batch  # noqa: E402

sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from gpu_common import TOL_BF16, TOL_FP32  # noqa: E402

SEED, B, D = 31, 16, 63
PERTURB = 1e-3
RED_DRAW_SEED = 3203      # one recorded draw for every RED-Diff case (per-case seeds 3200 + i: the draw of 3201 failed condition 3 at t = 0.3)


class StandIn:
    """What the reference's loss methods read from `self`; any other attribute is the reference class's own method, bound to this object."""

    def __init__(self, cls, model, sde, batch_size):
        self._cls = cls
        self.batch_size = batch_size
        self.sde = sde
        self.score_fn = ref_mutils.get_score_fn(sde, model, train=False, continuous=True)
        self.rsde = sde.reverse(self.score_fn, False)
        self.loss_fn = nn.MSELoss(reduction="none")

    def __getattr__(self, name):
        return types.MethodType(getattr(self._cls, name), self)


def rel(a, b):
    return float(torch.linalg.norm((a - b).double()) / torch.linalg.norm(b.double()))


def main():
    G._stub_finder()
    import run.motion_denoising as ref_md
    import run.smplify as ref_smplify
    cfg, m = build_model(SEED, D)
    m.eval()
    kinds = {"subvp": lambda: ref_sde.subVPSDE(0.1, 20.0, 1000), "vp": lambda: ref_sde.VPSDE(0.1, 20.0, 1000),
             "ve": lambda: ref_sde.VESDE(sigma_min=0.01, sigma_max=50.0, N=1000)}
    x0, _ = toy_batch(B, seed=131)
    out = {"seed": np.int64(SEED), "sigma_min": np.float64(0.01), "sigma_max": np.float64(50.0), "x0": x0.numpy(),
           "perturbation": np.float64(PERTURB)}

    def with_grad(fn, rec_seed):
        xv = x0.clone().requires_grad_(True)
        with Recorder(rec_seed) as rec:
            loss = fn(xv)
        loss.backward()
        return np.float64(loss.item()), xv.grad.numpy(), rec.by_kind("randn")[0]

    multi_cases = [("subvp", 0.3), ("subvp", 0.5), ("vp", 0.3), ("vp", 0.5), ("ve", 0.7)]
    red_cases = [("subvp", 0.1), ("subvp", 0.3), ("subvp", 0.5), ("vp", 0.1), ("vp", 0.3), ("vp", 0.5), ("ve", 0.3), ("ve", 0.7)]
    out["multi_cases"] = np.array([f"{k}_t{int(round(t * 10)):02d}" for k, t in multi_cases])
    out["red_cases"] = np.array([f"{k}_t{int(round(t * 10)):02d}" for k, t in red_cases])

    for ci, (kind, t) in enumerate(multi_cases):
        tag = f"multi_{kind}_t{int(round(t * 10)):02d}"
        sde = kinds[kind]()
        vec_t = torch.ones(B) * t
        rec_seed = 3100 + ci
        comp = StandIn(ref_completion.DPoserComp, m, sde, B)
        smp = StandIn(ref_smplify.DPoser, m, sde, B)
        md = StandIn(ref_md.MotionDenoise, m, sde, B)
        out[f"{tag}_t"] = np.float32(t)
        zs = []
        for name, fn in (("comp_w", lambda xv: comp.loss(xv, vec_t, weighted=True, multi_denoise=True)),
                         ("comp_u", lambda xv: comp.loss(xv, vec_t, weighted=False, multi_denoise=True)),
                         ("smplify", lambda xv: smp.DPoser_loss(xv, vec_t, multi_denoise=True)),
                         ("md", lambda xv: md.DPoser_loss(xv, vec_t, 0, weighted=False, multi_denoise=True))):
            loss, grad, z = with_grad(fn, rec_seed)
            out[f"{tag}_{name}_loss"], out[f"{tag}_{name}_grad"] = loss, grad
            zs.append(z)
        assert all(np.array_equal(zs[0], z) for z in zs)            # one recorded draw per case: every call perturbs with the same z
        z = torch.tensor(zs[0])
        out[f"{tag}_z"] = zs[0]
        with torch.no_grad():
            mean, std = sde.marginal_prob(x0, vec_t)
            x_t = mean + std[:, None] * z
            one, _ = comp.one_step_denoise(x_t, vec_t)
            tol = TOL_FP32 if kind == "ve" else TOL_BF16               # the loosest tolerance this case is tested at
            for N in (1, 5, 10):
                est, snr = comp.multi_step_denoise(x_t, vec_t, t_end=vec_t / (2 * N), N=N)
                out[f"{tag}_est{N}"] = est.numpy()
                d1, d2 = rel(est, one), rel(x0, est)
                out[f"{tag}_est{N}_dist_one_step"], out[f"{tag}_est{N}_x0_dist"] = np.float64(d1), np.float64(d2)
                print(f"{tag} N={N}: |est - one_step| / |one_step| = {d1:.3e}, |x0 - est| / |est| = {d2:.3f}")
                if N > 1:
                    assert d1 >= 5 * tol, (tag, N, d1, tol)          # condition 1
                assert d2 >= 0.5, (tag, N, d2)                       # condition 2
            out[f"{tag}_snr"] = np.float64(snr.reshape(-1)[0].item())

    for ci, (kind, t) in enumerate(red_cases):
        tag = f"red_{kind}_t{int(round(t * 10)):02d}"
        sde = kinds[kind]()
        vec_t = torch.ones(B) * t
        md = StandIn(ref_md.MotionDenoise, m, sde, B)
        loss, grad, z_np = with_grad(lambda xv: md.RED_Diff(xv, vec_t, 0), RED_DRAW_SEED)
        z = torch.tensor(z_np)
        out[f"{tag}_t"], out[f"{tag}_loss"], out[f"{tag}_grad"] = np.float32(t), loss, grad
        assert "red_z" not in out or np.array_equal(out["red_z"], z_np)
        out["red_z"] = z_np                                        # the one draw of every RED-Diff case
        with torch.no_grad():
            mean, std = sde.marginal_prob(x0, vec_t)
            _, _, alpha, sigma_2, score = md.rsde.sde(mean + std[:, None] * z, vec_t, guide=True)
            out[f"{tag}_eps_pred"] = (-score * std[:, None]).numpy()
            # condition 3 in float64: how far a relative error of the score moves the scalar
            s64, std64, z64, x64 = score.double(), std.double(), z.double(), x0.double()
            weight = torch.sqrt(sigma_2.double()) / alpha.double()[:, 0]
            scalar = lambda s: float(torch.mean(weight * torch.einsum("ij,ij->i", -s * std64[:, None] - z64, x64)))
            base = scalar(s64)
            signs = torch.tensor(np.random.RandomState(3300 + ci).choice([-1.0, 1.0], size=tuple(s64.shape)))
            amp = max(abs(scalar(s64 * (1 + PERTURB)) - base), abs(scalar(s64 * (1 + PERTURB * signs)) - base)) / abs(base) / PERTURB
        ok = amp <= 2.0
        expect_ok = not (kind in ("subvp", "vp") and t > 0.3)
        print(f"{tag}: scalar {base:.6e}, amplification of a {PERTURB:g} score error {amp:.3f}, scalar compared: {expect_ok}")
        assert abs(base - loss) <= 1e-5 * abs(base), (tag, base, loss)
        if expect_ok:
            assert ok, (tag, amp)                                   # condition 3
        out[f"{tag}_scalar_amplification"] = np.float64(amp)
        out[f"{tag}_scalar_ok"] = np.int64(1 if expect_ok else 0)
    save("g31_prior_variants", **out)


if __name__ == "__main__":
    main()
