"""Time the mesh self-intersection metric (dposer_mesh_self_intersections) at B in {1, 500, 4096} SMPL-sized meshes (F = 13776), with tile
culling and with every tile pair (DPOSER_SI_ALLPAIRS=1), next to the fp64 CPU oracle's time per mesh (tests/si_ref.py).

The meshes are posed copies of an 84 x 82 spindle torus (V = 6888, F = 13776, about 2 % of its faces self-intersect): random smooth
deformations, so every mesh differs.  Prints one line per (mode, B) and a JSON line."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,500,4096")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--oracle-meshes", type=int, default=2)
    ap.add_argument("--modes", default="culled,allpairs")
    args = ap.parse_args()
    import si_ref
    from dposer_amd import _C
    from dposer_amd.utils.metric import _mesh_si
    assert torch.cuda.is_available(), "si_time needs a GPU"
    X, F = si_ref.torus(r=1.3)
    base = np.stack([si_ref.smooth_deform(X, s) for s in range(16)])
    batches = [int(b) for b in args.batches.split(",")]
    Ft = torch.tensor(F, device="cuda")
    res = {"F": int(len(F)), "V": int(len(X))}
    for mode in args.modes.split(","):
        os.environ["DPOSER_SI_ALLPAIRS"] = "1" if mode == "allpairs" else "0"
        _C.lib().dposer_body_tuning_reload()
        rs = np.random.RandomState(0)                            # (the same meshes in every mode)
        torch.manual_seed(0)
        for B in batches:
            V = torch.tensor(base[rs.randint(0, 16, B)], device="cuda")
            V += 0.002 * torch.randn_like(V)
            flags, counts = _mesh_si(V, Ft)                     # warm-up
            torch.cuda.synchronize()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            for _ in range(args.reps):
                _mesh_si(V, Ft)
            ev[1].record()
            torch.cuda.synchronize()
            ms = ev[0].elapsed_time(ev[1]) / args.reps
            res[f"{mode}_B{B}_ms"] = ms
            print(f"{mode:9s} B={B:5d}  {ms:9.3f} ms/call  {ms / B * 1e3:8.2f} us/mesh  mean SI {counts.double().mean().item() / len(F) * 100:.3f} %",
                  flush=True)
    if args.oracle_meshes > 0:
        t = time.perf_counter()
        for k in range(args.oracle_meshes):
            si_ref.classify(base[k], F)
        res["oracle_s_per_mesh"] = (time.perf_counter() - t) / args.oracle_meshes
        print(f"fp64 CPU oracle: {res['oracle_s_per_mesh']:.3f} s/mesh")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
