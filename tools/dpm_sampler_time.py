#!/usr/bin/env python3
"""Times the few-step sampler (dposer_dpm_sampler: DPM-Solver++, 20 steps at order 2 on the logSNR grid) on one GPU and writes the sections
of profiles/dpm_sampler_time.md.  ScoreModelFC (H = 1024, 2 blocks, D = 63), sub-VP, no trajectory kept, B = 500 and B = 65536, all three
precisions.  Every mode appends its section to `--out`.

  (default)          time per call of the 20-step sampler, and dposer_em_sampler's time per step on the same build (N = `--em-steps` steps
                     of the one-launch-per-step form, no trajectory): device events around each call, one warm-up call, `--repeats` repeats
  --trace-leg        one warm-up call and one call per (precision, B), nothing else: the leg to run under
                     `rocprofv3 --kernel-trace --stats`, in a run of its own
  --from-trace DB    reads that run's rocpd database: k_dpm_update's share of the kernel time of a step, per (precision, B)
  --em-only          dposer_em_sampler alone at the largest B: the leg of the parent-versus-branch comparison.  `--lib PATH` times another
                     build of the library (an older one may lack the DPM entries: they are then left unbound); `--label` names the row.
                     Run the two builds in alternation, the parent's twice or more: the branch must lie inside the parent's own band.
"""
import argparse
import os
import sqlite3
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

DPM_STEPS, DPM_ORDER = 20, 2


def emit(out, text):
    print(text, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(text + "\n")


def from_trace(db, precisions, batches, out):
    """The kernels of the trace leg in start order; every run of DPM_STEPS k_dpm_update dispatches is one sampler call (warm-up, then the
    measured one, per precision and batch).  A step = the kernels behind the previous update (or behind the pack launch) up to its update."""
    cur = sqlite3.connect(db).cursor()
    cols = [r[1] for r in cur.execute("pragma table_info(kernels)")]
    name_col = "name" if "name" in cols else [c for c in cols if "name" in c][0]
    rows = list(cur.execute(f"select {name_col}, start, end from kernels order by start"))
    upd = [i for i, r in enumerate(rows) if "k_dpm_update" in r[0]]
    want = 2 * len(precisions) * len(batches) * DPM_STEPS
    assert len(upd) == want, f"{len(upd)} k_dpm_update dispatches in the trace, expected {want}"
    emit(out, "\n## k_dpm_update's share of a step (rocprofv3 --kernel-trace, a run of its own)\n")
    emit(out, "Kernel time only (gaps between kernels are not in it): per sampler call, the 20 update launches over all kernels from the first "
              "network GEMM to the last update.\n")
    emit(out, "| precision | B | kernel time per step, us | k_dpm_update per launch, us | share of a step |")
    emit(out, "|---|---:|---:|---:|---:|")
    call = 0
    for prec in precisions:
        for B in batches:
            call += 1                                   # skip the warm-up call
            idx = upd[call * DPM_STEPS:(call + 1) * DPM_STEPS]
            call += 1
            first = max(i for i in range(idx[0]) if "k_em_update" in rows[i][0]) + 1      # behind the imputation + pack launch
            tot = sum(e - s for _, s, e in rows[first:idx[-1] + 1])
            mine = sum(rows[i][2] - rows[i][1] for i in idx)
            emit(out, f"| {prec} | {B} | {tot / DPM_STEPS / 1e3:.1f} | {mine / DPM_STEPS / 1e3:.1f} | {100.0 * mine / tot:.1f} % |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[500, 65536])
    ap.add_argument("--precisions", nargs="+", default=["fp32", "bf16x3", "bf16"])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--em-steps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dpm_sampler_time.md"))
    ap.add_argument("--trace-leg", action="store_true")
    ap.add_argument("--from-trace", default=None)
    ap.add_argument("--em-only", action="store_true")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--label", default="this build")
    ap.add_argument("--offset-mb", type=int, default=0, help="hold this many MiB of device memory first: every later buffer moves, which "
                    "shows how much of a difference between two builds is where the buffers lie")
    a = ap.parse_args()
    if a.from_trace:
        return from_trace(a.from_trace, a.precisions, a.batches, a.out)
    if a.lib:
        os.environ["DPOSER_LIB_PATH"] = os.path.abspath(a.lib)
    import ctypes
    import torch
    from dposer_amd import _C
    if a.lib:                                           # an older build: leave unbound what it does not export
        probe = ctypes.CDLL(_C.LIB_PATH)
        for name in ("dposer_dpm_coefficients", "dposer_dpm_sampler"):
            if not hasattr(probe, name):
                _C.SIGNATURES.pop(name, None)
    from gpu_common import make_model
    from dposer_amd.algorithms.advanced import sampling, sde_lib
    assert torch.cuda.is_available(), "dpm_sampler_time.py measures on the GPU"
    dev = "cuda:0"
    hold = torch.empty(a.offset_mb << 20, dtype=torch.uint8, device=dev) if a.offset_mb else None      # noqa: F841 (kept allocated)

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        x = f()
        e1.record()
        torch.cuda.synchronize()
        assert torch.isfinite(x).all()
        return e0.elapsed_time(e1)

    def stats(ts, scale=1.0):
        return f"{statistics.median(ts) * scale:.3f} ({min(ts) * scale:.3f}-{max(ts) * scale:.3f})"

    def legs(m, B):
        z = torch.randn(B, 63, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
        sde = sde_lib.subVPSDE(0.1, 20.0, 1000)
        times = sampling.dpm_time_grid(sde, DPM_STEPS, "logSNR", 1e-3) if hasattr(sampling, "dpm_time_grid") else None
        sde_em = sde_lib.subVPSDE(0.1, 20.0, a.em_steps)
        ts_em = torch.linspace(sde_em.T, 1e-3, sde_em.N)
        dpm = lambda: sampling.fused_dpm_sample(m, sde, z, times, order=DPM_ORDER, traj_stride=0)[1]
        em = lambda: sampling.fused_em_sample(m, sde_em, z, ts_em, seed=2, traj_stride=0)[1]
        return dpm, em

    if a.trace_leg:
        for prec in a.precisions:
            _, m, _ = make_model(3, precision=prec)
            for B in a.batches:
                dpm, _ = legs(m, B)
                dpm(), dpm()
                torch.cuda.synchronize()
        return
    if a.em_only:
        B = max(a.batches)
        for prec in a.precisions:
            _, m, _ = make_model(3, precision=prec)
            _, em = legs(m, B)
            timed(em)
            ts = [timed(em) for _ in range(a.repeats)]
            emit(a.out, f"| {a.label} | {prec} | {B} | {a.em_steps} | {stats(ts, 1.0 / a.em_steps)} |")
        return
    emit(a.out, "# The few-step sampler (dposer_dpm_sampler) on one MI355X\n")
    emit(a.out, f"DPM-Solver++ (2M), {DPM_STEPS} steps at order {DPM_ORDER} on the logSNR grid, sub-VP, eps = 1e-3, ScoreModelFC (H = 1024, 2 blocks, "
                f"D = 63), no trajectory kept; device events around each call, one warm-up call, median (min-max) of {a.repeats} repeats.  "
                f"dposer_em_sampler on the same build: {a.em_steps} steps of its one-launch-per-step form, per step.  Written by "
                "tools/dpm_sampler_time.py.\n")
    emit(a.out, f"| precision | B | dposer_dpm_sampler, {DPM_STEPS} steps: ms per call | ms per step | dposer_em_sampler: ms per step | "
                "1000 Euler-Maruyama steps / 20 solver steps |")
    emit(a.out, "|---|---:|---:|---:|---:|---:|")
    for prec in a.precisions:
        _, m, _ = make_model(3, precision=prec)
        for B in a.batches:
            dpm, em = legs(m, B)
            timed(dpm), timed(em)
            td, te = [], []
            for _ in range(a.repeats):
                td.append(timed(dpm))
                te.append(timed(em))
            ratio = 1000.0 * statistics.median(te) / a.em_steps / statistics.median(td)
            emit(a.out, f"| {prec} | {B} | {stats(td)} | {statistics.median(td) / DPM_STEPS:.3f} | {stats(te, 1.0 / a.em_steps)} | {ratio:.1f}x |")


if __name__ == "__main__":
    main()
