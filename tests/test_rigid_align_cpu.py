"""CPU side of the rigid-alignment / EHF-evaluation feature: the fp64 rule of tests/align_ref.py against the reference's own outputs
(golden g29), the test-set generator's conditioning gate, compute_bbox / bbox_from_detector bit for bit, the PLY / OBJ readers, the new
reference import paths and the layout of the new argument structs."""
import os

import numpy as np
import pytest
import torch

import align_ref
from helpers import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIN = 1e-12        # both sides are fp64 numpy on gated inputs: they differ by summation order only (1e-16 x a conditioning of <= 1e2)


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300))


def test_align_ref_matches_the_reference_golden():
    g = load("g29_rigid_align")
    cases = [(g[f"ra{n}_src"][k], g[f"ra{n}_dst"][k], g[f"ra{n}_c"][k], g[f"ra{n}_R"][k], g[f"ra{n}_t"][k], g[f"ra{n}_aligned"][k])
             for n in (4, 22, 55) for k in range(len(g[f"ra{n}_src"])) if g[f"ra{n}_kept"][k]]
    cases += [tuple(g[f"hand_{nm}_{f}"] for f in ("src", "dst", "c", "R", "t", "aligned")) for nm in g["hand_names"]]
    assert len(cases) >= 100
    for A, B, c, R, t, aligned in cases:
        assert align_ref.conditioning(A, B) >= align_ref.CONDITION_GATE
        c2, R2, t2 = align_ref.similarity(A, B)
        assert abs(c2 - c) / c < PIN and _rel(R2, R) < PIN and _rel(t2, t) < PIN * 100     # (t = b - c R a cancels metres against metres)
        assert _rel(align_ref.align(A, B), aligned) < PIN
        assert abs(np.linalg.det(R) - 1) < 1e-12
    refl = np.concatenate([g[f"ra{n}_reflected"][g[f"ra{n}_kept"]] for n in (4, 22, 55)])
    assert refl.mean() >= 0.2                                  # the det R < 0 branch, asserted on the reference's own inputs
    assert align_ref.takes_reflection_branch(g["hand_mirrored_src"], g["hand_mirrored_dst"])


def test_align_ref_ehf_metrics_match_the_reference_golden():
    from dposer_amd.body_model.synthetic import make_synthetic_smplx_asset
    g = load("g29_rigid_align")
    J = make_synthetic_smplx_asset(seed=0)["J_regressor"]
    used = g["ehf_used_vertices"]
    assert np.array_equal(used, np.flatnonzero((J[:22] != 0).any(0)))
    for k in range(len(g["ehf_pa_mpjpe"])):
        pred, gt = np.zeros((J.shape[1], 3)), np.zeros((J.shape[1], 3))
        pred[used], gt[used] = g["ehf_pred_used"][k], g["ehf_gt_used"][k]
        pa, mp = align_ref.ehf_metrics(J, pred, gt, g["ehf_rotation"])
        assert abs(pa - g["ehf_pa_mpjpe"][k]) / g["ehf_pa_mpjpe"][k] < 1e-10     # (a mean of mm-sized distances between points metres away)
        assert abs(mp - g["ehf_mpjpe"][k]) / g["ehf_mpjpe"][k] < 1e-10


@pytest.mark.parametrize("n,count", [(4, 200), (22, 200), (55, 200), (64, 100), (65, 100), (10475, 10)])
def test_generated_sets_pass_the_conditioning_gate(n, count):
    src, dst = align_ref.kept_pairs(n, count, 1000 + n)
    assert src.dtype == np.float32 and src.shape[1:] == (n, 3) and len(src) >= 0.98 * count


def test_bbox_helpers_match_the_reference_bit_for_bit():
    from dposer_amd.utils.preprocess import bbox_from_detector, compute_bbox
    g = load("g29_rigid_align")
    kp = g["bbox_keypoints"]
    data = {"people": [{"pose_keypoints_2d": p.reshape(-1).tolist()} for p in kp]}
    out = compute_bbox(data)
    assert out.dtype == g["bbox_out"].dtype and np.array_equal(out, g["bbox_out"])
    assert list(out[:, 0]) == [0, 1, 3]                        # person 2 has no visible keypoint
    for bb, rescale, c, s in zip(g["bfd_boxes"], g["bfd_rescale"], g["bfd_center"], g["bfd_scale"]):
        center, scale = bbox_from_detector(torch.tensor(bb), float(rescale))
        assert center.dtype == torch.float64 and np.array_equal(center.numpy(), c) and float(scale) == s
    assert compute_bbox({"people": []}).shape == (0,)


@pytest.mark.parametrize("fmt", ["ascii", "binary_little_endian", "binary_big_endian"])
def test_ply_reader(tmp_path, fmt):
    from dposer_amd.utils.preprocess import load_ply
    rs = np.random.RandomState(5)
    v32 = rs.standard_normal((37, 3)).astype(np.float32)
    v64 = rs.standard_normal((37, 3))
    faces = [[0, 1, 2], [3, 4, 5, 6], [7, 8, 9]]
    extra = [("red", "uchar", rs.randint(0, 255, 37)), ("quality", "double", rs.standard_normal(37)), ("flag", "short", rs.randint(-9, 9, 37)),
             ("xy", "float", rs.standard_normal(37))]               # (a name made of coordinate letters is still another property)
    p = str(tmp_path / "m.ply")
    align_ref.write_ply(p, v32, fmt)
    out = load_ply(p)
    assert out.dtype == np.float32 and np.array_equal(out, v32)
    align_ref.write_ply(p, v64, fmt, dtype="double")
    out = load_ply(p)
    assert out.dtype == np.float64 and np.array_equal(out, v64)
    for faces_first in (False, True):
        align_ref.write_ply(p, v32, fmt, extra=extra, faces=faces, faces_first=faces_first)
        assert np.array_equal(load_ply(p), v32)
    # truncated body
    align_ref.write_ply(p, v32, fmt, faces=faces, faces_first=True)
    blob = open(p, "rb").read()
    body = blob.index(b"end_header\n") + len(b"end_header\n")
    for cut in (body + 5, body + (len(blob) - body) // 2):
        with open(p, "wb") as fh:
            fh.write(blob[:cut])
        with pytest.raises(ValueError, match="m.ply"):
            load_ply(p)


def test_ply_reader_rejects_bad_headers(tmp_path):
    from dposer_amd.utils.preprocess import load_ply
    p = str(tmp_path / "bad.ply")
    for text in (b"plx\nformat ascii 1.0\nend_header\n", b"ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\n",
                 b"ply\nformat binary_middle_endian 1.0\nelement vertex 0\nend_header\n",
                 b"ply\nformat ascii 1.0\nelement vertex 1\nproperty quaternion x\nend_header\n0\n",
                 b"ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float y\nend_header\n0 0\n",
                 b"ply\nformat ascii 1.0\nelement face 0\nproperty list uchar int vertex_indices\nend_header\n",
                 b"ply\nformat ascii 1.0\nelement vertex many\nproperty float x\nend_header\n",
                 b"ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float xy\nproperty float yz\nend_header\n0 0 0\n",
                 b"ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float y\nproperty float z\nend_header\n0 zero 0\n"):
        with open(p, "wb") as fh:
            fh.write(text)
        with pytest.raises(ValueError, match="bad.ply"):
            load_ply(p)


def test_load_obj(tmp_path):
    from dposer_amd.utils.preprocess import load_obj
    p = tmp_path / "m.obj"
    p.write_text("# a comment\nv 1.5 -2 3e-1\nvn 0 0 1\nv 4 5 6\nf 1 2 2\n")
    out = load_obj(str(p))
    assert out.dtype == np.float64 and np.array_equal(out, [[1.5, -2.0, 0.3], [4.0, 5.0, 6.0]])


def test_new_reference_import_paths():
    import dposer_amd
    dposer_amd.install_reference_aliases()
    from lib.dataset.mocap_dataset import MocapDataset
    from lib.utils.preprocess import bbox_from_detector, compute_bbox, load_obj, load_ply  # noqa: F401
    from lib.utils.transforms import rigid_align, rigid_transform_3D  # noqa: F401
    import dposer_amd.dataset.mocap_dataset as ours
    assert MocapDataset is ours.MocapDataset and callable(rigid_align) and callable(compute_bbox)
    for name in ("eval_EHF", "eval_EHF_batch", "print_eval_result", "__getitem__"):
        assert callable(getattr(MocapDataset, name))
    import dposer_amd.tasks.fitting as fitting
    assert callable(fitting.initial_fit) and callable(fitting.fit_and_evaluate) and callable(fitting.run_folder)


def test_run_folder_refuses_files_that_do_not_pair_up(tmp_path):
    import json
    import types
    from dposer_amd.tasks.fitting import run_folder
    sm = types.SimpleNamespace(smpl=types.SimpleNamespace(mean_poses=torch.zeros(72)))
    for k in range(2):
        (tmp_path / f"{k:02d}_2Djnt.json").write_text(json.dumps({"people": [{"pose_keypoints_2d": [0.0] * 75}]}))
    align_ref.write_ply(str(tmp_path / "00_align.ply"), np.zeros((3, 3), np.float32))
    with pytest.raises(ValueError, match="do not pair up"):                       # a ground-truth mesh is missing
        run_folder(str(tmp_path), str(tmp_path / "out"), sm, None, image_shapes=[(8, 8), (8, 8)])
    align_ref.write_ply(str(tmp_path / "02_align.ply"), np.zeros((3, 3), np.float32))
    with pytest.raises(ValueError, match="do not pair up"):                       # same count, another image's mesh
        run_folder(str(tmp_path), str(tmp_path / "out"), sm, None, image_shapes=[(8, 8), (8, 8)])
    os.rename(tmp_path / "02_align.ply", tmp_path / "01_align.ply")
    with pytest.raises(ValueError, match="do not pair up"):
        run_folder(str(tmp_path), str(tmp_path / "out"), sm, None, image_shapes=[(8, 8)])
    with pytest.raises(ValueError, match="00_2Djnt.json: no person with a visible keypoint"):
        run_folder(str(tmp_path), str(tmp_path / "out"), sm, None, image_shapes=[(8, 8), (8, 8)], bend_pose_path=str(tmp_path / "none.npz"))


def test_host_arrays_need_a_gpu_not_a_cpu_path():
    """There is no CPU arithmetic path: device functions refuse CPU tensors."""
    from dposer_amd import _C
    from dposer_amd.utils.transforms import rigid_align_device
    with pytest.raises(_C.DPoserHipError):
        rigid_align_device(torch.zeros(1, 4, 3), torch.zeros(1, 4, 3))


def test_new_args_structs_match_the_header_layout(tmp_path):
    """dposer_rigid_align_args / dposer_regress_joints_args / dposer_ehf_eval_args as the C compiler lays them out against their ctypes
    mirrors: size and the offset of every field (the check test_host_cpu.py applies to the older structs)."""
    import ctypes as C
    import shutil
    import subprocess
    from dposer_amd import _C
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    pairs = {"dposer_rigid_align_args": _C.RigidAlignArgs, "dposer_regress_joints_args": _C.RegressJointsArgs,
             "dposer_ehf_eval_args": _C.EhfEvalArgs}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dposer_hip.h"', 'int main(void) {']
    for cname, ct in pairs.items():
        lines.append(f'  printf("{cname} size %zu\\n", sizeof({cname}));')
        for fname, _ in ct._fields_:
            lines.append(f'  printf("{cname} {fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ['  return 0;', '}']
    src = tmp_path / "abi_probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "abi_probe"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = {}
    for ln in subprocess.check_output([str(exe)], text=True).splitlines():
        a, b, c = ln.split()
        got[(a, b)] = int(c)
    for cname, ct in pairs.items():
        assert got[(cname, "size")] == C.sizeof(ct), cname
        for fname, _ in ct._fields_:
            assert got[(cname, fname)] == getattr(ct, fname).offset, (cname, fname)


def test_capi_rejects_bad_alignment_arguments():
    """Argument checks of the new entries run on the host before anything is launched."""
    from dposer_amd import _C
    lib = _C.lib()
    assert lib.dposer_rigid_align(None, None) < 0 and b"NULL" in lib.dposer_last_error()
    a = _C.RigidAlignArgs(None, None, 4, 0, None, None, None)
    assert lib.dposer_rigid_align(a, None) < 0 and b"num_points" in lib.dposer_last_error()
    a = _C.RigidAlignArgs(None, None, 4, 22, None, None, None)
    assert lib.dposer_rigid_align(a, None) < 0 and b"src and dst" in lib.dposer_last_error()
    assert lib.dposer_rigid_align(_C.RigidAlignArgs(None, None, 0, 22, None, None, None), None) == 0          # empty batch: nothing to do
    r = _C.RegressJointsArgs(None, 2, 100, None, None, None, 22, None)
    assert lib.dposer_regress_joints(r, None) < 0 and b"required" in lib.dposer_last_error()
    e = _C.EhfEvalArgs(None, None, 2, 100, None, None, None, 22, None, 22, None, None, None, None, None, None)
    assert lib.dposer_ehf_eval(e, None) < 0 and b"pelvis_row" in lib.dposer_last_error()
    assert lib.dposer_ehf_eval_scratch_bytes(100, 22) >= 2 * 100 * 22 * 12 + 400 and lib.dposer_ehf_eval_scratch_bytes(-1, 22) == 0
