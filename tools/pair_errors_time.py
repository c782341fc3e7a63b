#!/usr/bin/env python
"""Times Evaler.multi_eval_bodys with fused=False and fused=True on one GPU and writes profiles/pair_errors_time.md.

Grid: B in {1024, 4096, 16384} x H in {1, 5} x part in {None, "legs", "left_leg"}, on the default SMPL-X-shaped synthetic asset and on
the same asset with coherent_skinning=True.  Per case, in one process: both paths warmed up, then timed in alternating windows (device
events around a window that ends in a synchronise), repetitions chosen so that a window lasts about --window seconds; the peak of
torch.cuda.max_memory_allocated above what was allocated before the case; the two front calls and the pair-error kernels of the fused
path timed on their own; the bytes the fused kernels must move, from the shapes.

    python tools/pair_errors_time.py [--out profiles/pair_errors_time.md] [--window 0.4] [--batches 1024 4096 16384]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12          # bytes/s, MI355X data sheet


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
    fn()                                                            # warm-up: allocator, lazily built tables
    torch.cuda.synchronize()
    one = window(fn, 2)
    return int(min(max(np.ceil(seconds / max(one, 1e-6)), 3), 2000))


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def fused_bytes(core, B, H, n, m):
    """What the two pair-error kernels must move: offsets and transforms of both bodies over the listed vertices, the per-wave partial
    sums out and back, the joint rows, the tables once."""
    nblk = -(-n // 256)
    per_body = n * 12 + core.J * 48 + m * 12
    return B * (1 + H) * per_body + 2 * B * H * nblk * 16 + n * (12 + 32) + 8 * B


def run_asset(name, asset, args, lines):
    from dposer_amd.body_model.body_model import BodyModel
    from dposer_amd.dataset.AMASS import Evaler
    from dposer_amd.utils import metric
    dev = "cuda:0"
    bm = BodyModel(asset).to(dev)
    core = bm.bm
    lines += [f"## {name}", "",
              "| B | H | part | verts | unfused ms | fused ms | unfused / fused | unfused peak MB | fused peak MB | fronts ms (share of fused) | "
              "kernels ms | kernel GB | kernel GB/s (of 8 TB/s) |", "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    rs = np.random.RandomState(0)
    for B in args.batches:
        gts = torch.tensor((rs.standard_normal((B, 63)) * 0.3).astype(np.float32), device=dev)
        for H in args.hypotheses:
            outs = (gts[:, None] + 0.1 * torch.randn(B, H, 63, device=dev)).contiguous()
            for part in (None, "legs", "left_leg"):
                ev = Evaler(bm, part=part)
                n = core.V if part is None else ev._vert_list.n
                m = core.J + core.n_extra + core.n_lmk if part is None else ev._row_list.n
                paths = {"unfused": lambda: ev.multi_eval_bodys(outs, gts, as_tensors=True, fused=False),
                         "fused": lambda: ev.multi_eval_bodys(outs, gts, as_tensors=True, fused=True)}
                t, peak = {}, {}
                for k, fn in paths.items():
                    core._ws = None                                  # (the unfused forward keeps its workspace: part of its footprint)
                    try:
                        peak[k] = peak_of(fn)
                        reps = reps_for(fn, args.window)
                        t[k] = (fn, reps, [])
                    except torch.cuda.OutOfMemoryError:
                        peak[k], t[k] = None, None
                        torch.cuda.empty_cache()
                for _ in range(3):                                   # alternating windows
                    for k in paths:
                        if t[k] is not None:
                            t[k][2].append(window(t[k][0], t[k][1]))
                ms = {k: (None if t[k] is None else 1e3 * float(np.median(t[k][2]))) for k in paths}
                # the fused path's two halves on their own
                hyp_rows = outs.reshape(B * H, 63)
                fronts = lambda: (core.lbs_front(body_pose=gts), core.lbs_front(body_pose=hyp_rows))
                fr_ms = 1e3 * float(np.median([window(fronts, reps_for(fronts, args.window / 2)) for _ in range(2)]))
                ref, hyp = fronts()
                o1, o2 = torch.empty(B, device=dev), torch.empty(B, device=dev)
                kern = lambda: metric._score_fronts(core, ref, hyp, H, ev._vert_list, ev._row_list, 1000.0, False, o1, o2)
                k_ms = 1e3 * float(np.median([window(kern, reps_for(kern, args.window / 2)) for _ in range(2)]))
                del ref, hyp
                nbytes = fused_bytes(core, B, H, n, m)
                f = lambda x, fmt: "does not fit" if x is None else fmt.format(x)
                ratio = None if ms["unfused"] is None else ms["unfused"] / ms["fused"]
                lines.append(f"| {B} | {H} | {part} | {n} | {f(ms['unfused'], '{:.3f}')} | {ms['fused']:.3f} | {f(ratio, '{:.2f}')} | "
                             f"{f(None if peak['unfused'] is None else peak['unfused'] / 2**20, '{:.0f}')} | {peak['fused'] / 2**20:.0f} | "
                             f"{fr_ms:.3f} ({100 * fr_ms / ms['fused']:.0f} %) | {k_ms:.3f} | {nbytes / 1e9:.3f} | "
                             f"{nbytes / (k_ms / 1e3) / 1e9:.0f} ({100 * nbytes / (k_ms / 1e3) / HBM_PEAK:.0f} %) |")
                print(lines[-1], flush=True)
    lines.append("")
    del bm
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair_errors_time.md"))
    ap.add_argument("--window", type=float, default=0.4, help="seconds per timing window")
    ap.add_argument("--batches", type=int, nargs="+", default=[1024, 4096, 16384])
    ap.add_argument("--hypotheses", type=int, nargs="+", default=[1, 5])
    ap.add_argument("--notes", default=None, help="a text file appended to the report (what was read off the table)")
    args = ap.parse_args()
    from dposer_amd.body_model.synthetic import make_synthetic_smplx_asset
    lines = ["# Pose-pair errors: Evaler.multi_eval_bodys, fused=False against fused=True", "",
             f"One {torch.cuda.get_device_name(0)}, torch {torch.__version__}; written by tools/pair_errors_time.py.  Times are medians of three "
             f"alternating windows of about {args.window} s per path, device events around a window that ends in a synchronise, every shape warmed up.  "
             "Peak MB: torch.cuda.max_memory_allocated above what was allocated before the case.  fronts: the two dposer_lbs_forward_front "
             "calls (FK + pose-blend GEMM over all 3V columns) of the fused path; kernels: dposer_pose_pair_errors alone on prepared workspaces; "
             "kernel GB: offsets and transforms of both bodies over the listed vertices, partial sums, joint rows, tables once.", ""]
    run_asset("default synthetic SMPL-X asset (random skinning joints)", make_synthetic_smplx_asset(seed=0), args, lines)
    run_asset("coherent_skinning=True", make_synthetic_smplx_asset(seed=0, coherent_skinning=True), args, lines)
    if args.notes:
        lines += open(args.notes).read().rstrip("\n").split("\n") + [""]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
