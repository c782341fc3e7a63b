"""Time the batched rigid alignment (dposer_rigid_align) and the one-call EHF evaluation (dposer_ehf_eval) next to the per-sample host path
the reference takes (device -> host copy of the data, fp64 numpy per sample: tests/align_ref.py), alternating the two in one process.

    python tools/align_time.py                   # the table of profiles/align_time.md
    python tools/align_time.py --trace-only      # 5 dposer_ehf_eval calls at B = 100: the workload of the rocprofv3 listing

Device-event times after warm-up over windows of about 250 ms (up to 10000 calls); the host path is timed with the host clock around work
that ends on the host.  Bytes per call are the algorithmic ones, from the shapes: alignment reads src and dst twice (moments, then outputs) and writes what is asked for; the evaluation
reads the vertices its regressor rows name and moves kilobytes of joints.  Prints one line per case and a JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _window_ms(fn, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1])


def device_ms(fn, window_ms=250.0):
    """ms per call over a window of about ``window_ms`` of device time (20 to 10000 calls, sized from a 20-call probe after warm-up)."""
    fn()
    torch.cuda.synchronize()
    reps = int(min(10000, max(20, window_ms / max(_window_ms(fn, 20) / 20, 1e-6))))
    return _window_ms(fn, reps) / reps


def host_ms(fn, reps):
    fn()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3, help="alternations of (one call, host loop) per case")
    ap.add_argument("--host-samples", type=int, default=100, help="samples of the host loop that are actually run (its time scales with B)")
    ap.add_argument("--trace-only", action="store_true")
    args = ap.parse_args()
    import align_ref
    from dposer_amd.body_model.synthetic import make_synthetic_smplx_asset
    from dposer_amd.dataset.mocap_dataset import ehf_eval, regressor_csr
    from dposer_amd.utils.transforms import batch_rodrigues, rigid_align_device
    assert torch.cuda.is_available(), "align_time needs a GPU"
    dev = "cuda"
    gen = torch.Generator(device=dev).manual_seed(0)
    J = make_synthetic_smplx_asset(seed=0)["J_regressor"]
    csr = regressor_csr(J, 22, dev)
    nnz = int(csr[0][-1])
    rot = batch_rodrigues(torch.tensor([[-2.98747896, 0.01172457, -0.05704687]], device=dev))[0]
    Rn = rot.cpu().numpy().astype(np.float64)

    def meshes(B, V):
        a = torch.randn(B, V, 3, device=dev, generator=gen) * torch.tensor([0.4, 0.25, 0.1], device=dev) + torch.tensor([1.0, -2.0, 3.0], device=dev)
        b = a.flip(2) * 1.2 + 0.03 * torch.randn(B, V, 3, device=dev, generator=gen)
        return a, b

    if args.trace_only:
        a, b = meshes(100, J.shape[1])
        for _ in range(5):
            ehf_eval(a, b, csr, rot, 0)
        torch.cuda.synchronize()
        return

    res = {}
    print("case                          one call        host loop (per-sample copy + fp64 numpy)   algorithmic bytes/call")
    for N, B in ((22, 100), (22, 4096), (22, 65536), (10475, 100), (10475, 4096)):
        a, b = meshes(B, N)
        n_host = min(B, args.host_samples)

        def host():
            for k in range(n_host):
                align_ref.mean_distance(align_ref.align(a[k].cpu().numpy(), b[k].cpu().numpy()), b[k].cpu().numpy())

        one, loop = [], []
        for _ in range(args.rounds):
            one.append(device_ms(lambda: rigid_align_device(a, b)))
            loop.append(host_ms(host, 1) * B / n_host)
        nbytes = B * (N * 12 * 5 + 13 * 4 + 4)
        res[f"align_N{N}_B{B}"] = dict(one_call_ms=min(one), one_call_ms_all=one, host_loop_ms=min(loop), host_samples_run=n_host, bytes=nbytes)
        print(f"rigid_align N={N:5d} B={B:5d}  {min(one):9.4f} ms   {min(loop):11.2f} ms ({n_host} samples run, scaled)   {nbytes / 1e6:10.3f} MB"
              f"   {nbytes / min(one) / 1e6:8.1f} GB/s", flush=True)
    V = J.shape[1]
    for B in (100, 4096):
        a, b = meshes(B, V)
        n_host = min(B, args.host_samples)

        def host():
            for k in range(n_host):
                align_ref.ehf_metrics(J, a[k].cpu().numpy(), b[k].cpu().numpy(), Rn)

        one, loop = [], []
        for _ in range(args.rounds):
            one.append(device_ms(lambda: ehf_eval(a, b, csr, rot, 0)))
            loop.append(host_ms(host, 1) * B / n_host)
        nbytes = B * (2 * nnz * 12 + 22 * 12 * 2 * 3 + 8) + nnz * 8
        res[f"ehf_eval_B{B}"] = dict(one_call_ms=min(one), one_call_ms_all=one, host_loop_ms=min(loop), host_samples_run=n_host, bytes=nbytes)
        print(f"ehf_eval V={V} B={B:5d}     {min(one):9.4f} ms   {min(loop):11.2f} ms ({n_host} samples run, scaled)   {nbytes / 1e6:10.3f} MB", flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
