"""Time the mesh renderer (dposer_render_meshes through body_model.visual.render_meshes) at B in {1, 500, 4096} meshes, one image each,
in the two setups of the reference's visual.py, next to the fp64 CPU oracle's time per image (tests/render_ref.py).

Cases:
    torus_demo     a closed deformed torus of SMPL-X size (106 x 99 grid: V = 10494, F = 20988), 1.7 m tall, render_mesh's scene
                   (512 x 384, focal 1500, principal point (200, 192), flat shading, three lights, random views per mesh);
    torus_faster   the same meshes in faster_render's scene (256 x 256, 60-degree field of view, smooth shading, one point light);
    synthetic_demo the synthetic SMPL-X asset (random face triples: nearly every face lands on the large list) in render_mesh's scene.
The time is between device events around --reps calls after one warm-up call; it includes the host side of render_meshes (input checks:
one device sync for the face index range; the vertex -> face CSR in smooth mode).  Prints one line per (case, B) and a JSON line."""
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
    ap.add_argument("--synthetic-batches", default="1,500")
    ap.add_argument("--cases", default="torus_demo,torus_faster,synthetic_demo")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--oracle-images", type=int, default=2)
    args = ap.parse_args()
    import render_ref
    import si_ref
    from dposer_amd.body_model import visual
    assert torch.cuda.is_available(), "render_time needs a GPU"
    dev = "cuda"
    X, F = si_ref.torus(n_u=106, n_v=99, R=0.6, r=0.25)
    X = (X * np.array([0.8, 1.0, 1.0], np.float32)).astype(np.float32)
    base = np.stack([si_ref.smooth_deform(X, s, amp=0.05) for s in range(16)])
    from dposer_amd.body_model.synthetic import make_synthetic_smplx_asset
    asset = make_synthetic_smplx_asset(seed=0)
    syn_v, syn_f = np.asarray(asset["v_template"], np.float32), np.asarray(asset["faces"], np.int64)
    rs = np.random.RandomState(0)
    views = ["front", "left", "right", "back", "half_left", "half_right_above", "bottom", "above"]
    res = {"torus_F": int(len(F)), "torus_V": int(len(X)), "synthetic_F": int(len(syn_f))}
    Kd = [1500.0, 1500.0, 200.0, 192.0]
    Tf, Kf = visual.faster_camera()
    light_f = Tf[:, :3] @ np.array([0.0, 0.0, 3.0]) + Tf[:, 3]
    for case in args.cases.split(","):
        batches = args.synthetic_batches if case.startswith("synthetic") else args.batches
        for B in [int(b) for b in batches.split(",")]:
            if case.startswith("synthetic"):
                V = np.broadcast_to(syn_v, (B,) + syn_v.shape)
                faces = syn_f
            else:
                V = base[rs.randint(0, 16, B)]
                faces = F
            Vt = torch.tensor(np.ascontiguousarray(V), device=dev)
            Ft = torch.tensor(faces, device=dev)
            if case == "torus_faster":
                kw = dict(intrinsics=torch.tensor(Kf, dtype=torch.float32, device=dev), image_size=(256, 256),
                          transforms=torch.tensor(Tf, dtype=torch.float32, device=dev), lights=[(1, *light_f, 0.3, 0.3, 0.3)], ambient=0.5,
                          smooth=True, background_color=(255, 255, 255), znear=1.0, zfar=100.0)
            else:
                cent = V.astype(np.float64).mean(1)
                T = np.stack([visual.render_mesh_transform(cent[b], *visual.parse_view(views[b % len(views)])) for b in range(B)])
                kw = dict(intrinsics=torch.tensor([Kd], device=dev), image_size=(512, 384), transforms=torch.tensor(T, dtype=torch.float32, device=dev),
                          base_color=visual.RENDER_MESH_COLOR, lights=[(0, 0, 0, -1, *[visual.RENDER_MESH_LIGHT] * 3)] * 3,
                          ambient=visual.RENDER_MESH_AMBIENT)
            out = visual.render_meshes(Vt, Ft, outputs=("rgb", "depth"), **kw)                 # warm-up
            torch.cuda.synchronize()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            for _ in range(args.reps):
                visual.render_meshes(Vt, Ft, outputs=("rgb", "depth"), **kw)
            ev[1].record()
            torch.cuda.synchronize()
            ms = ev[0].elapsed_time(ev[1]) / args.reps
            cov = (out["depth"] > 0).float().sum(dim=(1, 2)).mean().item()
            res[f"{case}_B{B}_ms"] = ms
            print(f"{case:15s} B={B:5d}  {ms:9.3f} ms/call  {ms / B * 1e3:9.2f} us/image  {cov:9.0f} covered px/image", flush=True)
            del out, Vt
            torch.cuda.empty_cache()
    if args.oracle_images > 0:
        t = time.perf_counter()
        for k in range(args.oracle_images):
            T = visual.render_mesh_transform(base[k].astype(np.float64).mean(0), 0, 0)
            render_ref.render(base[k][None], F, Kd, 512, 384, transforms=T[None].astype(np.float32), base_color=visual.RENDER_MESH_COLOR,
                              lights=[(0, 0, 0, -1, *[visual.RENDER_MESH_LIGHT] * 3)] * 3, ambient=visual.RENDER_MESH_AMBIENT)
        res["oracle_s_per_image"] = (time.perf_counter() - t) / args.oracle_images
        print(f"fp64 CPU oracle (torus_demo): {res['oracle_s_per_image']:.3f} s/image")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
