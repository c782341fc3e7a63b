"""Timings behind profiles/feed_time.md: (a) dposer_batch_gather against torch.index_select with the indices already on the device,
(b) tasks.train.train()'s time per step against the same step on one fixed batch and against the reference's way of feeding it (a shuffling
DataLoader over AMASSDataset, four workers, one host-to-device copy per step).

    python tools/feed_time.py [--out FILE] [--skip-loader]

Needs a GPU.  Device events around windows of back-to-back calls for (a); for (b) the host clock between points where the device has been
synchronised (train()'s log points are such points: the window's sums are read back there).  Runs that are compared alternate in one process.
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda:0"
N_ROWS = 1 << 22


def event_window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(calls):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls                        # ms per call


def gather_table(emit):
    from dposer_amd.dataset.feed import DeviceFeed
    emit("## (a) The gather: `dposer_batch_gather` against `torch.index_select`\n")
    emit("| D | B | index_select, 5 rounds (min - max) | batch_gather, 5 rounds (min - max) | ratio of medians | bytes moved / gather time |")
    emit("|---:|---:|---:|---:|---:|---:|")
    for D in (63, 126):
        data = torch.randn(N_ROWS, D, device=DEV)
        for B in (1280, 8192, 65536):
            feed = DeviceFeed(data, B, seed=3, num_replicas=1, rank=0)
            K = min(feed.steps_per_epoch, 64)
            idx = [feed.indices(s) for s in range(K)]       # the baseline's indices: the same rows, already on the device
            pos = [feed.position(s) for s in range(K)]
            out = torch.empty(B, D, device=DEV)

            def base(i):
                torch.index_select(data, 0, idx[i % K], out=out)

            def ours(i):
                e, b0 = pos[i % K]
                feed.gather(e, b0, B, out=out)

            ours(0)
            assert torch.equal(out, data[idx[0]])
            calls = max(200, int(60.0 / max(event_window(base, 50), 1e-3)))           # about 60 ms per window
            tb, to = [], []
            for _ in range(5):                              # alternate; the baseline twice per round shows its own spread
                tb.append(event_window(base, calls))
                to.append(event_window(ours, calls))
                tb.append(event_window(base, calls))
            mb, mo = float(np.median(tb)), float(np.median(to))
            gbs = 2 * B * D * 4 / (mo * 1e-3) / 1e9
            emit(f"| {D} | {B} | {mb * 1e3:.1f} us ({min(tb) * 1e3:.1f} - {max(tb) * 1e3:.1f}) | {mo * 1e3:.1f} us ({min(to) * 1e3:.1f} - "
                 f"{max(to) * 1e3:.1f}) | {mo / mb:.2f} | {gbs:.0f} GB/s |")
        del data
    emit("")


class DeviceSet:
    def __init__(self, poses):
        self.poses = poses

    def Denormalize(self, poses, shapes=None):
        return poses


def _config(B):
    from dposer_amd.configs import load_config
    cfg = load_config("configs.subvp.amass_scorefc_continuous.get_config")
    cfg.training.batch_size = B
    cfg.training.log_freq = 50
    cfg.training.eval_freq = cfg.training.save_freq = 10 ** 9
    return cfg


def _windows(stamps):
    """ms per step of the 50-step windows between synchronised time stamps, the first two windows dropped (warm-up)."""
    w = np.diff(np.array(stamps)) / 50 * 1e3
    return w[2:]


def train_run(cfg, train_set, n_iters, out_dir):
    from dposer_amd.tasks.train import train
    stamps = []

    def log(msg):
        if msg.startswith("Iter: ["):
            stamps.append(time.perf_counter())

    train(cfg, train_set, DeviceSet(train_set.poses[:50]), None, out_dir, n_iters=n_iters, log=log)
    return _windows(stamps)


def _state_and_step(cfg):
    from dposer_amd.algorithms.advanced import losses
    from dposer_amd.algorithms.ema import ExponentialMovingAverage
    from dposer_amd.tasks.train import build_model, build_sde
    model = build_model(cfg).to(DEV)
    state = dict(optimizer=losses.get_optimizer(cfg, model.parameters()), model=model,
                 ema=ExponentialMovingAverage(model.parameters(), decay=cfg.model.ema_rate), step=0)
    fn = losses.get_step_fn(build_sde(cfg)[0], train=True, optimize_fn=losses.optimization_manager(cfg), reduce_mean=True, continuous=True)
    model.train()
    return state, fn


def fixed_run(cfg, batch, n_iters):
    """The same step on one fixed device tensor, synchronised every 50 steps like train()'s log points."""
    state, fn = _state_and_step(cfg)
    stamps = []
    for s in range(n_iters):
        fn(state, batch)
        if (s + 1) % 50 == 0:
            torch.cuda.synchronize()
            stamps.append(time.perf_counter())
    return _windows(stamps)


def loader_run(cfg, dataset, n_iters):
    """run/train.py:79-84, 247-249: a shuffling DataLoader with four workers and a host-to-device copy per step."""
    from torch.utils.data import DataLoader
    state, fn = _state_and_step(cfg)
    loader = DataLoader(dataset, batch_size=cfg.training.batch_size, shuffle=True, num_workers=4, pin_memory=False, drop_last=True)
    stamps, s = [], 0
    while s < n_iters:
        for item in loader:
            fn(state, item["poses"].to(DEV, non_blocking=True))
            s += 1
            if s % 50 == 0:
                torch.cuda.synchronize()
                stamps.append(time.perf_counter())
            if s >= n_iters:
                break
    return _windows(stamps)


def fmt(w):
    return f"{np.median(w):.3f} ms ({w.min():.3f} - {w.max():.3f}, {len(w)} windows)"


def loop_table(emit, skip_loader):
    emit("## (b) The loop: `train()` per step against the step on one fixed batch\n")
    emit("| poses per step | `train()` (feed + step + device-side loss sums) | fixed batch (step alone) | ratio of medians |")
    emit("|---:|---:|---:|---:|")
    poses = torch.randn(N_ROWS, 63, device=DEV)
    train_set = DeviceSet(poses)
    med = {}
    with tempfile.TemporaryDirectory() as tmp:
        for B, n_iters in ((1280, 2000), (65536, 500)):
            cfg = _config(B)
            fixed = poses[:B].clone()
            wt, wf = [], []
            for _ in range(2):                              # alternate the two, two rounds each
                wt.append(train_run(cfg, train_set, n_iters, tmp))
                wf.append(fixed_run(cfg, fixed, n_iters))
            wt, wf = np.concatenate(wt), np.concatenate(wf)
            med[B] = float(np.median(wf))
            emit(f"| {B} | {fmt(wt)} | {fmt(wf)} | {np.median(wt) / np.median(wf):.3f} |")
        emit("")
        if skip_loader:
            return
        from dposer_amd.dataset.AMASS import AMASSDataset
        n = 1 << 18
        os.makedirs(os.path.join(tmp, "v", "train"))
        torch.save(torch.randn(n, 63) * 0.3, os.path.join(tmp, "v", "train", "pose_body.pt"))
        ds = AMASSDataset(tmp, version="v", subset="train", rot_rep="axis", normalize=True, min_max=False)
        w = loader_run(_config(1280), ds, 600)
        emit("| feed of the step at 1280 poses | time per step |")
        emit("|---|---:|")
        emit(f"| `DataLoader(batch_size=1280, shuffle=True, num_workers=4, drop_last=True)` over `AMASSDataset` ({n} rows) + H2D copy | {fmt(w)} |")
        emit(f"| the same step on one fixed batch (from the table above) | {med[1280]:.3f} ms |")
        emit("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-loader", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("feed_time.py measures on a GPU; none found (no CPU fallback, no numbers)")
    fh = open(args.out, "w") if args.out else None

    def emit(line):
        print(line, flush=True)
        if fh:
            fh.write(line + "\n")
            fh.flush()

    emit(f"device: {torch.cuda.get_device_name(0)}, dataset rows: {N_ROWS}\n")
    gather_table(emit)
    loop_table(emit, args.skip_loader)


if __name__ == "__main__":
    main()
