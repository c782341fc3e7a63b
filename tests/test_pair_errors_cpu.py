"""CPU side of the pose-pair error feature (dposer_pose_pair_errors / utils.metric.pose_pair_errors / Evaler(fused=True)): the float64
rule of tests/pair_err_ref.py against the reference's own evaluator (golden g18), the layout of the argument struct, the argument checks
of the C entry (they run before any launch) and the host-side checks of the Python layer."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import pair_err_ref
from helpers import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def asset():
    from dposer_amd.body_model.synthetic import make_synthetic_smplx_asset
    return make_synthetic_smplx_asset(seed=0)


@pytest.fixture(scope="module")
def g18_ref(asset):
    """The float64 rule on the golden's poses, once for all parts: the bodies are rounded to fp32 once, as the golden's are."""
    g = load("g18_evaler")
    B, H = g["outs"].shape[:2]
    vr, jr = pair_err_ref.bodies(asset, g["gts"], round_fp32=True)
    hyp = [pair_err_ref.bodies(asset, g["outs"][:, h], round_fp32=True) for h in range(H)]
    return g, vr, jr, hyp


@pytest.mark.parametrize("part", pair_err_ref.PARTS)
def test_pair_err_ref_reproduces_the_reference_evaluator(part, asset, g18_ref):
    """golden g18 = lib/dataset/AMASS.py:263-316 on fp64 bodies rounded to fp32, reduced in fp32; here the same bodies reduced in fp64:
    1e-6 of the largest value (a mean of <= 10475 fp32 terms)."""
    g, vr, jr, hyp = g18_ref
    vi, ji = pair_err_ref.part_lists(part)
    sel = lambda x, idx: x if idx is None else x[:, idx]
    ev = np.stack([np.sqrt(((sel(v, vi) - sel(vr, vi)) ** 2).sum(-1)).mean(-1) * 1000 for v, _ in hyp], 1)
    ej = np.stack([np.sqrt(((sel(j, ji) - sel(jr, ji)) ** 2).sum(-1)).mean(-1) * 1000 for _, j in hyp], 1)
    tag = part or "all"
    for got, key in ((ev.min(1), "mpvpe_all"), (ej.min(1), "mpjpe_body"), (ev[:, 0], "h0_mpvpe_all"), (ej[:, 0], "h0_mpjpe_body")):
        want = g[f"{tag}/{key}"]
        assert np.abs(got - want).max() / np.abs(want).max() < 1e-6, (part, key)
    if part == "legs":                                             # the packaged function is the same arithmetic
        r = pair_err_ref.pair_errors(asset, g["gts"], g["outs"], vi, ji, scale=1000.0, round_fp32=True)
        assert np.array_equal(r["mpvpe"], ev.min(1)) and np.array_equal(r["mpjpe_h"], ej)


def test_pair_err_ref_minimum_keeps_a_nan():
    x = np.zeros((2, 21 * 3))
    hyp = np.zeros((2, 3, 63))
    hyp[1, 1, 4] = np.nan
    from dposer_amd.body_model.synthetic import make_synthetic_smplx_asset
    r = pair_err_ref.pair_errors(make_synthetic_smplx_asset(seed=0, num_vertices=300), x, hyp, vert_idx=[0, 5], joint_idx=[5])    # (joint 5 hangs below the NaN rotation of joint 2)
    assert r["mpvpe"][0] == 0.0 and np.isnan(r["mpvpe"][1]) and np.isnan(r["mpjpe"][1])


def test_pose_pair_errors_args_match_the_header_layout(tmp_path):
    """dposer_pose_pair_errors_args as the C compiler lays it out against its ctypes mirror and against the offsets the header documents."""
    import re
    from dposer_amd import _C
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    cname, ct = "dposer_pose_pair_errors_args", _C.PosePairErrorsArgs
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dposer_hip.h"', 'int main(void) {',
             f'  printf("size %zu\\n", sizeof({cname}));']
    lines += [f'  printf("{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in ct._fields_]
    lines += ['  return 0;', '}']
    src = tmp_path / "abi_probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "abi_probe"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict((a, int(b)) for a, b in (ln.split() for ln in subprocess.check_output([str(exe)], text=True).splitlines()))
    assert got["size"] == C.sizeof(ct)
    for f, _ in ct._fields_:
        assert got[f] == getattr(ct, f).offset, f
    # the header's own statement of the layout
    hdr = open(os.path.join(ROOT, "include", "dposer_hip.h")).read()
    body = hdr[hdr.index("typedef struct dposer_pose_pair_errors_args {"):hdr.index("} dposer_pose_pair_errors_args;")]
    stated = {m.group(1): int(m.group(2)) for m in re.finditer(r"(\w+);\s*/\*\s*(\d+)", body)}
    assert stated == {f: got[f] for f, _ in ct._fields_}
    assert f"sizeof = {got['size']}" in hdr


@pytest.fixture(scope="module")
def body_handle():
    from dposer_amd import _C
    from dposer_amd.body_model.synthetic import make_synthetic_smplx_asset
    par = np.asarray(make_synthetic_smplx_asset(seed=0, num_vertices=300)["parents"]).astype(np.int32)
    desc = _C.BodyDesc(55, 300, 20, 21, 51)
    h = C.c_void_p()
    assert _C.lib().dposer_body_create(C.byref(desc), (C.c_int32 * 55)(*[int(p) for p in par]), C.byref(h)) == 0
    yield h
    _C.lib().dposer_body_destroy(h)


def test_capi_rejects_bad_pair_error_arguments(body_handle):
    """Every argument check of dposer_pose_pair_errors returns a negative status and a message before anything is launched: the pointers
    are fakes, nothing here touches a device."""
    from dposer_amd import _C
    lib = _C.lib()
    A, S = 0x100000, 0x100040                                      # 256-byte aligned / not aligned fake addresses

    def args(**kw):
        base = dict(body=body_handle, ws_ref=A, ws_hyp=A, joints_ref=A, joints_hyp=A, v_shaped=A, v_shaped_batched=0, skin_k=4, skin_idx=A, skin_w=A,
                    transl_ref=None, transl_hyp=None, vert_list=None, joint_rows=None, num_listed_vertices=0, num_listed_rows=0, max_listed_row=0,
                    hypotheses=3, extra_vertex_ids=A, lmk_tri=A, lmk_bary=A, batch=4, scale=1000.0, min_into=0, mpvpe=A, mpjpe=A, mpvpe_h=None,
                    mpjpe_h=None, scratch=A)
        base.update(kw)
        return _C.PosePairErrorsArgs(**base)

    def rejected(word, **kw):
        rc = lib.dposer_pose_pair_errors(C.byref(args(**kw)), None)
        msg = lib.dposer_last_error()
        assert rc < 0 and word in msg, (kw, rc, msg)

    assert lib.dposer_pose_pair_errors(None, None) < 0 and b"NULL" in lib.dposer_last_error()
    for name in ("body", "ws_ref", "ws_hyp", "joints_ref", "joints_hyp", "v_shaped", "skin_idx", "skin_w", "scratch"):
        rejected(b"null argument", **{name: None})
    for name in ("mpvpe", "mpjpe"):
        rejected(b"null output", **{name: None})
    rejected(b">= 1", batch=0)
    rejected(b">= 1", hypotheses=0)
    rejected(b">= 1", skin_k=0)
    rejected(b"num_listed_vertices", vert_list=A, num_listed_vertices=0)
    rejected(b"num_listed_rows", joint_rows=A, num_listed_rows=0)
    rejected(b"4096", joint_rows=A, num_listed_rows=4097, max_listed_row=3)
    for name in ("ws_ref", "ws_hyp", "scratch"):
        rejected(b"256-byte aligned", **{name: S})
    rejected(b"max_listed_row", joint_rows=A, num_listed_rows=2, max_listed_row=127)
    rejected(b"max_listed_row", joint_rows=A, num_listed_rows=2, max_listed_row=-1)
    rejected(b"extra_vertex_ids", extra_vertex_ids=None)                                      # all rows: the extras are listed
    rejected(b"extra_vertex_ids", joint_rows=A, num_listed_rows=2, max_listed_row=55, extra_vertex_ids=None)
    rejected(b"lmk_tri", lmk_tri=None)
    rejected(b"lmk_tri", joint_rows=A, num_listed_rows=2, max_listed_row=76, lmk_bary=None)
    rejected(b"2^31", batch=1 << 40)
    # scratch size: one float per (sample, hypothesis, 256-entry block, wave), rounded up to 256 bytes
    assert lib.dposer_pose_pair_errors_scratch_bytes(body_handle, 4, 3, 0) == 512                # 4 x 3 x 2 blocks x 16 bytes = 384
    assert lib.dposer_pose_pair_errors_scratch_bytes(body_handle, 1, 1, 1) == 256
    assert lib.dposer_pose_pair_errors_scratch_bytes(body_handle, 0, 3, 0) < 0 and lib.dposer_pose_pair_errors_scratch_bytes(None, 4, 3, 0) < 0


def test_fused_paths_need_a_gpu_not_a_cpu_path(asset):
    from dposer_amd import _C
    from dposer_amd.body_model.body_model import BodyModel
    from dposer_amd.dataset.AMASS import Evaler
    from dposer_amd.utils.metric import pose_pair_errors
    bm = BodyModel(asset)
    ref, hyp = torch.zeros(2, 63), torch.zeros(2, 3, 63)
    with pytest.raises(_C.DPoserHipError):
        pose_pair_errors(bm, ref, hyp)
    for part in ("legs", None):
        ev = Evaler(bm, part=part)
        with pytest.raises(_C.DPoserHipError):
            ev.eval_bodys(hyp[:, 0], ref, fused=True)
        with pytest.raises(_C.DPoserHipError):
            ev.multi_eval_bodys(hyp, ref, fused=True)


def test_index_lists_are_range_checked_on_the_host():
    from dposer_amd.body_model.body_model import BodyModel
    from dposer_amd.body_model.synthetic import make_synthetic_smplx_asset
    from dposer_amd.utils.metric import IndexList, pose_pair_errors
    bm = BodyModel(make_synthetic_smplx_asset(seed=0, num_vertices=300))
    ref, hyp = torch.zeros(2, 63), torch.zeros(2, 3, 63)
    for kw in (dict(vert_idx=[0, 300]), dict(vert_idx=[-1]), dict(joint_idx=[127]), dict(joint_idx=torch.tensor([0, -2])), dict(vert_idx=[]),
               dict(vert_idx=np.zeros((2, 2), np.int64)), dict(joint_idx=[0.5]), dict(vert_idx=IndexList([0, 1], 10475))):
        with pytest.raises(ValueError):
            pose_pair_errors(bm, ref, hyp, **kw)
    lst = IndexList(torch.tensor([299, 0, 7]), 300)
    assert (lst.n, lst.max, lst.host.dtype) == (3, 299, np.int32)
