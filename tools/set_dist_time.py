#!/usr/bin/env python
"""Times the pose-set distance scores (dposer_pose_set_distances behind utils.metric) on one GPU and writes profiles/set_dist_time.md.

Rows: APD of B = 500 / 8192 / 65536 poses of 22 joints, average_pairwise_distance_hip against the torch average_pairwise_distance (the
APD of the commit before this feature, unchanged since) in alternating windows -- the torch path is reported as "does not fit", with the
bytes of its [chunk, B, J, 3] intermediate, where it runs out of memory; the 3 nearest of 2^20 references for 65536 poses;
generation_fidelity at 8192 x 8192; and single calls at 8192 x 8192 that show what each output costs.  Random data (the generator of
tests/set_dist_ref.py), every shape warmed up, medians of alternating windows, device events around a window that ends in a synchronise,
no profiler.  Beside each time: the pair-joints the score needs (from the shapes) per second, as a share of the VALU issue floor of
include/dposer_hip.h's cost note (256 CUs x 4 SIMDs x 64 lanes / 36 cycles x 2 GHz = 3.6e12 pair-joints/s).

    python tools/set_dist_time.py [--out profiles/set_dist_time.md] [--window 0.3] [--notes notes.md]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FLOOR = 256 * 4 * 64 / 36 * 2.0e9          # pair-joints/s: one (pair, joint) = 36 issue cycles per wave, at 2 GHz
DEV = "cuda:0"


def window(fn, reps):
    """Seconds per call over one window of `reps` calls."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / 1e3 / reps


def reps_for(fn, seconds):
    fn()
    fn()                                                            # warm-up: code objects, allocator
    torch.cuda.synchronize()
    one = window(fn, 1)
    return int(min(max(np.ceil(seconds / max(one, 1e-6)), 2), 2000))


def timed(paths, seconds, rounds=3):
    """{name: median seconds per call} over `rounds` alternating windows; a path that runs out of memory maps to None."""
    plan = {}
    for name, fn in paths.items():
        try:
            plan[name] = (fn, reps_for(fn, seconds), [])
        except torch.cuda.OutOfMemoryError:
            plan[name] = None
            torch.cuda.empty_cache()
    for _ in range(rounds):
        for name, p in plan.items():
            if p is not None:
                p[2].append(window(p[0], p[1]))
    return {name: (None if p is None else float(np.median(p[2]))) for name, p in plan.items()}


def poses(n, J, seed):
    """The generator of tests/set_dist_ref.py, on the device."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    base = 0.3 * torch.randn(J, 3, generator=g)
    scale = 0.5 + torch.rand(n, 1, 1, generator=g)
    return (base[None] * scale + 0.05 * torch.randn(n, J, 3, generator=g)).float().to(DEV)


def rate(pair_joints, seconds):
    r = pair_joints / seconds
    return f"{r:.3g} ({100 * r / FLOOR:.0f} %)"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "set_dist_time.md"))
    ap.add_argument("--window", type=float, default=0.3, help="seconds per timing window")
    ap.add_argument("--apd", type=int, nargs="+", default=[500, 8192, 65536])
    ap.add_argument("--queries", type=int, default=65536)
    ap.add_argument("--references", type=int, default=1 << 20)
    ap.add_argument("--fidelity", type=int, default=8192)
    ap.add_argument("--notes", default=None, help="a text file appended to the report (what was read off the tables)")
    args = ap.parse_args()
    from dposer_amd.utils import metric as M
    J = 22
    lines = ["# Pose-set distances: APD, nearest neighbours and fidelity scores in one kernel family", "",
             f"One {torch.cuda.get_device_name(0)}, torch {torch.__version__}; the tables are written by tools/set_dist_time.py.  Random poses of {J} "
             f"joints (the generator of tests/set_dist_ref.py), every shape warmed up, medians of three alternating windows of about {args.window} s "
             "per path (at least two calls), device events around a window that ends in a synchronise, no profiler.  pair-joints: what the score "
             "needs, from the shapes (the symmetric APD counts each unordered pair once); the share is of the derived VALU issue floor "
             f"256 CUs x 4 SIMDs x 64 lanes / 36 cycles x 2 GHz = {FLOOR:.2e} pair-joints/s (include/dposer_hip.h, cost note).", "",
             "## APD: average_pairwise_distance_hip against the torch average_pairwise_distance", "",
             "| B | torch ms | hip ms | torch / hip | torch intermediate [1024, B, J, 3] | pair-joints | pair-joints/s (share of floor) |",
             "|---|---|---|---|---|---|---|"]
    for B in args.apd:
        x = poses(B, J, B)
        t = timed({"torch": lambda: M.average_pairwise_distance(x), "hip": lambda: M.average_pairwise_distance_hip(x)}, args.window)
        inter = min(1024, B) * B * J * 3 * 4
        pj = B * (B - 1) // 2 * J
        agree = ""
        if t["torch"] is not None:
            a, b = float(M.average_pairwise_distance(x)), float(M.average_pairwise_distance_hip(x))
            agree = f" (values agree to {abs(a - b) / a:.1e})"
        lines.append(f"| {B} | " + (f"{1e3 * t['torch']:.3f}" if t["torch"] is not None else "does not fit") + f" | {1e3 * t['hip']:.3f} | "
                     + (f"{t['torch'] / t['hip']:.1f}" if t["torch"] is not None else "-") + f" | {inter / 1e9:.2f} GB{agree} | {pj:.3g} | "
                     f"{rate(pj, t['hip'])} |")
        print(lines[-1], flush=True)
        del x
        torch.cuda.empty_cache()
    lines += ["", "## Nearest neighbours and fidelity", "", "| call | ms | pair-joints | pair-joints/s (share of floor) |", "|---|---|---|---|"]
    q, ref = poses(args.queries, J, 1), poses(args.references, J, 2)
    t = timed({"knn": lambda: M.nearest_pose_distance(q, ref, k=3)}, args.window)["knn"]
    pj = args.queries * args.references * J
    lines.append(f"| nearest_pose_distance, k = 3, {args.queries} poses against {args.references} references | {1e3 * t:.1f} | {pj:.3g} | {rate(pj, t)} |")
    print(lines[-1], flush=True)
    del q, ref
    torch.cuda.empty_cache()
    n = args.fidelity
    G, R = poses(n, J, 3), poses(n, J, 4)
    t = timed({"fid": lambda: M.generation_fidelity(G, R, k=3)}, args.window)["fid"]
    pj = (4 * n * n + n * (n - 1) // 2) * J                        # two radius calls, two cross calls, one symmetric sum
    lines.append(f"| generation_fidelity, k = 3, {n} generated against {n} real (five calls) | {1e3 * t:.2f} | {pj:.3g} | {rate(pj, t)} |")
    print(lines[-1], flush=True)
    lines += ["", f"## What each output costs: single calls, {n} x {n}", "", "| call | ms | pair-joints | pair-joints/s (share of floor) |",
              "|---|---|---|---|"]
    radii = M.pose_set_distances(R, k=3)["knn_dist"][:, 2].contiguous()
    G23, R23 = poses(n, 23, 5), poses(n, 23, 6)
    singles = {"sum, full form (two sets)": (lambda: M.pose_set_distances(G, R, want_sum=True), n * n * J),
               "sum, symmetric form (one set)": (lambda: M.pose_set_distances(G, want_sum=True), n * (n - 1) // 2 * J),
               "k = 1": (lambda: M.pose_set_distances(G, R, k=1), n * n * J),
               "k = 3": (lambda: M.pose_set_distances(G, R, k=3), n * n * J),
               "k = 8": (lambda: M.pose_set_distances(G, R, k=8), n * n * J),
               "covered": (lambda: M.pose_set_distances(G, R, radii=radii), n * n * J),
               "k = 1 + covered + sum": (lambda: M.pose_set_distances(G, R, k=1, radii=radii, want_sum=True), n * n * J),
               "k = 3, forced splits = 1": (lambda: M.pose_set_distances(G, R, k=3, splits=1), n * n * J),
               "k = 3, 23 joints (general path)": (lambda: M.pose_set_distances(G23, R23, k=3), n * n * 23)}
    ts = timed({name: fn for name, (fn, _) in singles.items()}, args.window / 2)
    for name, (_, pj) in singles.items():
        lines.append(f"| {name} | {1e3 * ts[name]:.3f} | {pj:.3g} | {rate(pj, ts[name])} |")
        print(lines[-1], flush=True)
    lines.append("")
    if args.notes:
        lines += open(args.notes).read().rstrip("\n").split("\n") + [""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
