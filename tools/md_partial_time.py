"""What partial observations (joints_conf / obs_joints, k_md_joint_obs) cost the one-call motion-denoising loop per Adam step.

    python3 tools/md_partial_time.py --out profiles/md_partial_time.md
    rocprofv3 --kernel-trace --stats -d out -o md -- python3 tools/md_partial_time.py --only none,left_leg --sizes 128    (the two kernels'
        own times, a run of its own; then python3 tools/rocpd_summary.py out/.../md_results.db)

Sizes: 128 x 60 and 1 x 60 frames (config 5 and config 5 x 128).  Paths: joints_conf = None (the yardstick: k_md_joint, the kernels of every call
before the feature), explicit ones, the left leg occluded (NaN under c = 0), head and wrists only (obs_joints = [15, 20, 21]).  A window is one
``optimize_sequences`` call between two device events, ended by a synchronise; the time per step is the SLOPE between a long and a short
window, (t(long) - t(short)) / (steps(long) - steps(short)), so the fixed cost of a call (ground truth, smoothing, metrics) drops out.  Every
shape is warmed up; three rounds alternate over the paths (yardstick first and last in every round) and the medians are reported, with the
spread between the two yardstick windows of the same rounds.  Profiler off."""
import argparse
import os
import statistics
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from dposer_amd.algorithms.advanced.model import ScoreModelFC
from dposer_amd.body_model.body_model import BodyModel
from dposer_amd.body_model.synthetic import make_synthetic_smplx_asset
from dposer_amd.configs import load_config
from dposer_amd.dataset.AMASS import Posenormalizer
from dposer_amd.tasks.motion_denoising import MotionDenoise
from dposer_amd.utils.misc import occlude_joints

F = 60
PATHS = ("none", "ones", "left_leg", "sparse3")
LONG, SHORT = (2, 50), (2, 10)                 # (iterations, steps per iteration): 100 and 20 Adam steps


def setup(dev):
    cfg = load_config("configs.subvp.amass_scorefc_continuous.get_config")
    torch.manual_seed(0)
    model = ScoreModelFC(cfg, n_poses=21, pose_dim=3, hidden_dim=1024, embed_dim=512, n_blocks=2).to(dev).eval()
    toy = torch.tensor(np.load(os.path.join(ROOT, "tests", "golden", "g10_normalizer.npz"))["toy_pose_samples"]).float()
    stats = {"mean_poses": toy.mean(0), "std_poses": toy.std(0) + 1e-3, "min_poses": toy.min(0).values, "max_poses": toy.max(0).values}
    norm = Posenormalizer(stats, device=dev, normalize=True, min_max=False, rot_rep="axis")
    bm = BodyModel(make_synthetic_smplx_asset(seed=0), batch_size=F).to(dev)
    args = types.SimpleNamespace(device=dev, dataset_folder="", version="", task="denoise")
    md = MotionDenoise(cfg, args, model, bm, sde_N=1000, batch_size=F, normalizer=norm)
    gt = toy[torch.arange(F) % len(toy)].to(dev) + 0.02 * torch.randn(F, 63, device=dev)
    return md, bm, gt


def problem(md, bm, gt, S, path, dev):
    """(joints3d [S, F, n_obs, 3], gt [S, F, 63], init [S, F, 63], keyword arguments of the path)."""
    gb = gt[None].expand(S, -1, -1).contiguous() + 0.01 * torch.randn(S, F, 63, device=dev)
    with torch.no_grad():
        jt = bm(pose_body=gb.reshape(S * F, 63), betas=md.betas[:1].expand(S * F, -1).contiguous()).Jtr
    rows = [15, 20, 21] if path == "sparse3" else list(range(22))
    j = (jt[:, rows] + 0.04 * torch.randn(S * F, len(rows), 3, device=dev)).reshape(S, F, len(rows), 3)
    kw = {}
    if path == "ones":
        kw = {"joints_conf": torch.ones(S, F, 22, device=dev)}
    elif path == "left_leg":
        j, conf = occlude_joints(j, part="left_leg")
        kw = {"joints_conf": conf}
    elif path == "sparse3":
        kw = {"obs_joints": rows}
    return j, gb, gb + 0.05 * torch.randn(S, F, 63, device=dev), kw


def window(md, prob, steps):
    j, gb, init, kw = prob
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    md.optimize_sequences(j, gb, time_strategy="3", iterations=steps[0], steps_per_iter=steps[1], init_poses=init, **kw)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="write the markdown report here as well")
    ap.add_argument("--sizes", default="128,1", help="sequences per call, comma separated")
    ap.add_argument("--only", default=None, help="run these paths alone (comma separated), one short and one long window per size, no report (for a kernel trace)")
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the timing needs a GPU"
    dev = torch.device("cuda", 0)
    md, bm, gt = setup(dev)
    sizes = [int(s) for s in a.sizes.split(",")]
    if a.only:
        only = a.only.split(",")
        assert all(p in PATHS for p in only), only
        for S in sizes:
            for p in only:
                prob = problem(md, bm, gt, S, p, dev)
                window(md, prob, SHORT)
                window(md, prob, LONG)
        return
    n_long, n_short = LONG[0] * LONG[1], SHORT[0] * SHORT[1]
    lines = ["# Partial observations in the one-call motion-denoising loop: time per Adam step", "",
             f"`tools/md_partial_time.py` on {torch.cuda.get_device_name(0)}.  Per size and path: the median over {a.rounds} rounds of "
             f"(t({n_long} steps) - t({n_short} steps)) / {n_long - n_short}, device events around `optimize_sequences` calls that end in a synchronise, every shape "
             "warmed up, the paths alternating inside a round, profiler off.  `none` (joints_conf = None, obs_joints = None) runs `k_md_joint` and is "
             "the yardstick; it is timed twice per round (first and last), and the spread is the largest difference between those two windows' "
             "per-step times over the rounds.", ""]
    for S in sizes:
        probs = {p: problem(md, bm, gt, S, p, dev) for p in PATHS}
        for p in PATHS:                              # warm up every shape and both window lengths
            window(md, probs[p], SHORT)
            window(md, probs[p], LONG)
        order = ("none",) + PATHS[1:] + ("none_again",)
        per_step = {p: [] for p in order}
        call_ms = {p: [] for p in order}
        for _ in range(a.rounds):
            for p in order:
                prob = probs["none" if p == "none_again" else p]
                t_short, t_long = window(md, prob, SHORT), window(md, prob, LONG)
                per_step[p].append((t_long - t_short) / (n_long - n_short))
                call_ms[p].append(t_long)
        med = {p: statistics.median(v) for p, v in per_step.items()}
        yard = statistics.median(per_step["none"] + per_step["none_again"])
        spread = max(abs(x - y) for x, y in zip(per_step["none"], per_step["none_again"]))
        lines += [f"## {S} x {F} frames", "",
                  f"yardstick `none`: {yard * 1e3:.1f} us per step (median of both windows of every round); spread between its two windows: "
                  f"{spread * 1e3:.2f} us = {100 * spread / yard:.2f} %", "",
                  "| path | us per step (median) | rounds, us per step | vs yardstick us | vs yardstick % | beyond the spread | ms per 100-step call (median) |",
                  "|---|---:|---|---:|---:|---|---:|"]
        for p in order:
            diff = med[p] - yard
            lines.append(f"| `{p}` | {med[p] * 1e3:.1f} | {' '.join(f'{x * 1e3:.1f}' for x in per_step[p])} | {diff * 1e3:+.2f} | {100 * diff / yard:+.2f} | "
                         f"{'yes' if abs(diff) > spread else 'no'} | {statistics.median(call_ms[p]):.2f} |")
        lines.append("")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
