"""CPU side of the skeleton plots and the motion video (csrc/draw.hip, body_model/visual.py, utils/motion_video.py): the reference's import
paths, the C ABI of the two new entry points, the AVI container, the frozen colour table, the oracle's own agreement with the reference's
recorded ``resize_or_crop`` / ``crop_bottom``, and the depth-key gap of the seeds the GPU tests draw."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

import skeleton_ref
from helpers import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# seeds of tests/test_gpu_draw.py's random sequences, per batch size
SEQUENCE_SEEDS = {1: (0, 1), 60: (1, 7)}
KEY_GAP = 1e-4


def test_reference_import_lines_resolve():
    """run/motion_denoising.py:14,21 with the aliases installed."""
    import dposer_amd
    dposer_amd.install_reference_aliases()
    from lib.body_model.visual import faster_render, render_mesh, save_obj, vis_skeletons  # noqa: F401
    from lib.utils.motion_video import seq_to_video
    from lib.utils.transforms import get_rotation_matrix_x, get_rotation_matrix_y, rotate_points
    from dposer_amd.body_model import visual
    from dposer_amd.utils import motion_video
    assert vis_skeletons is visual.vis_skeletons and seq_to_video is motion_video.seq_to_video
    p = np.array([[1.0, 2.0, 3.0]])
    assert np.allclose(rotate_points(p, get_rotation_matrix_x(np.pi)), [[1.0, -2.0, -3.0]])
    assert np.allclose(rotate_points(p, get_rotation_matrix_y(np.pi / 2)), [[3.0, 2.0, -1.0]])
    from dposer_amd.tasks.generation import generation_process  # noqa: F401
    from dposer_amd.tasks.motion_denoising import MotionDenoise
    assert isinstance(MotionDenoise.__dict__["visualize"], staticmethod)


def test_draw_symbols_are_declared_exported_and_mirrored():
    from dposer_amd import _C
    names = ("dposer_draw_skeletons", "dposer_draw_skeletons_scratch_bytes", "dposer_compose_panels")
    out = subprocess.check_output(["nm", "-D", "--defined-only", _C.LIB_PATH], text=True)
    syms = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    header = open(os.path.join(ROOT, "include", "dposer_hip.h")).read()
    for n in names:
        assert n in _C.SIGNATURES and n in syms and n + "(" in header, n
    assert f"#define DPOSER_MAX_PANELS {_C.MAX_PANELS}\n" in header
    assert f"#define DPOSER_DRAW_MAX_PRIMITIVES {_C.DRAW_MAX_PRIMITIVES}\n" in header
    l = _C.lib()
    assert l.dposer_draw_skeletons_scratch_bytes(4096, 22, 21) == 4096 * 43 * 32
    assert l.dposer_draw_skeletons_scratch_bytes(1, 4000, 97) == 0                     # more primitives than one call takes
    # argument checks return before anything is launched
    a = _C.DrawSkeletonsArgs(batch=1, num_joints=1, num_bones=0, height=0, width=4)
    assert l.dposer_draw_skeletons(a, None) != 0 and b"height" in l.dposer_last_error()
    c = _C.ComposeArgs(num_panels=9, num_frames=1, out_h=4, out_w=4)
    assert l.dposer_compose_panels(c, None) != 0 and b"num_panels" in l.dposer_last_error()


def test_draw_structs_match_the_header_layout(tmp_path):
    """The new argument structs as gcc lays them out against their ctypes mirrors (the method of
    test_host_cpu.py::test_ctypes_structs_match_the_header_layout): size and the offset of every field."""
    import ctypes as C
    from dposer_amd import _C
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    pairs = {"dposer_draw_skeletons_args": _C.DrawSkeletonsArgs, "dposer_panel": _C.Panel, "dposer_compose_args": _C.ComposeArgs}
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


@pytest.mark.parametrize("width", [1, 5, 6, 7, 8, 53])
def test_video_round_trip_is_bit_exact(tmp_path, width):
    """Widths whose 24-bit rows need 1, 2, 3 and no padding bytes."""
    from dposer_amd.utils.motion_video import read_video, write_video
    rs = np.random.RandomState(width)
    frames = rs.randint(0, 256, (5, 9, width, 3)).astype(np.uint8)
    path = write_video(str(tmp_path / "clip.mp4"), frames, 20)
    assert path == str(tmp_path / "clip.avi") and os.path.exists(path) and not os.path.exists(str(tmp_path / "clip.mp4"))
    back, fps = read_video(path)
    assert back.dtype == np.uint8 and np.array_equal(back, frames) and fps == 20.0
    # a tensor, an .avi path and a fractional rate
    path2 = write_video(str(tmp_path / "t.avi"), torch.as_tensor(frames), 29.97)
    back2, fps2 = read_video(path2)
    assert path2.endswith("t.avi") and np.array_equal(back2, frames) and abs(fps2 - 29.97) < 1e-9
    with pytest.raises(ValueError):
        write_video(str(tmp_path / "bad.avi"), frames.astype(np.float32), 20)


def test_video_file_follows_the_avi_layout(tmp_path):
    """The file parsed by hand: RIFF 'AVI ' { LIST hdrl { avih, LIST strl { strh vids / DIB, strf BITMAPINFOHEADER } }, LIST movi { 00db x N },
    idx1 } with every size, the frame count, the rate and the index offsets (counted from the 'movi' fourcc) landing on '00db'."""
    from dposer_amd.utils.motion_video import write_video
    N, H, W, fps = 4, 6, 7, 30
    frames = np.random.RandomState(3).randint(0, 256, (N, H, W, 3)).astype(np.uint8)
    d = open(write_video(str(tmp_path / "v.avi"), frames, fps), "rb").read()
    u32 = lambda at: struct.unpack_from("<I", d, at)[0]
    stride = 24                                                                   # 7 * 3 = 21 bytes padded to a multiple of 4
    fb = stride * H
    assert d[0:4] == b"RIFF" and u32(4) == len(d) - 8 and d[8:12] == b"AVI "
    at = 12
    assert d[at:at + 4] == b"LIST" and d[at + 8:at + 12] == b"hdrl"
    hdrl_end = at + 8 + u32(at + 4)
    at += 12
    assert d[at:at + 4] == b"avih" and u32(at + 4) == 56
    avih = struct.unpack_from("<14I", d, at + 8)
    assert avih[0] == 33333 and avih[3] & 0x10 and avih[4] == N and avih[6] == 1 and avih[7] == fb and avih[8:10] == (W, H)
    at += 8 + 56
    assert d[at:at + 4] == b"LIST" and d[at + 8:at + 12] == b"strl" and at + 8 + u32(at + 4) == hdrl_end
    at += 12
    assert d[at:at + 4] == b"strh" and u32(at + 4) == 56 and d[at + 8:at + 16] == b"vidsDIB "
    scale, rate, start, length = struct.unpack_from("<4I", d, at + 8 + 20)
    assert rate / scale == fps and start == 0 and length == N
    assert struct.unpack_from("<4h", d, at + 8 + 48) == (0, 0, W, H)
    at += 8 + 56
    assert d[at:at + 4] == b"strf" and u32(at + 4) == 40
    bi = struct.unpack_from("<IiiHHIIiiII", d, at + 8)
    assert bi[:7] == (40, W, H, 1, 24, 0, fb)                                     # positive height: bottom-up rows; BI_RGB
    at += 8 + 40
    assert at == hdrl_end
    assert d[at:at + 4] == b"LIST" and u32(at + 4) == 4 + N * (8 + fb) and d[at + 8:at + 12] == b"movi"
    movi = at + 8
    at += 12
    for i in range(N):
        assert d[at:at + 4] == b"00db" and u32(at + 4) == fb
        rows = np.frombuffer(d, np.uint8, fb, at + 8).reshape(H, stride)
        assert np.array_equal(rows[:, :W * 3].reshape(H, W, 3), frames[i, ::-1, :, ::-1]) and not rows[:, W * 3:].any()
        at += 8 + fb
    assert d[at:at + 4] == b"idx1" and u32(at + 4) == 16 * N and at + 8 + 16 * N == len(d)
    for i in range(N):
        cc, flags, off, size = struct.unpack_from("<4sIII", d, at + 8 + 16 * i)
        assert cc == b"00db" and flags & 0x10 and size == fb
        assert d[movi + off:movi + off + 4] == b"00db" and movi + off == movi + 4 + i * (8 + fb)


def test_colour_table_and_joint_colours():
    """The frozen table is the documented formula; discs take the colour of the last bone that touches them."""
    from dposer_amd.body_model import visual
    from dposer_amd.body_model.utils import get_smpl_skeleton
    grid = np.linspace(0.0, 1.0, 256)
    lut = np.clip(np.stack([np.abs(2 * grid - 0.5), np.sin(np.pi * grid), np.cos(np.pi * grid / 2)], 1), 0.0, 1.0)
    x = np.linspace(0.0, 1.0, 23)[:21]
    want = np.rint(lut[np.minimum((x * 256).astype(int), 255)][:, ::-1] * 255).astype(np.uint8)
    table = np.asarray(visual.SKELETON_COLORS_21, np.uint8)
    assert np.array_equal(table, want) and np.array_equal(visual.rainbow_swapped(21), table)
    assert tuple(table[0]) == (255, 0, 128)                                      # rainbow starts at purple (0.5, 0, 1): swapped
    assert visual.rainbow_swapped(5).shape == (5, 3)
    bones = get_smpl_skeleton()
    jc = visual.skeleton_joint_colors(bones, table, 22)
    for j in range(22):
        last = max(k for k in range(len(bones)) if j in bones[k])
        assert tuple(jc[j]) == tuple(table[last])
    s, X0, Y0, cx, cy = visual.skeleton_view([-1.0, 0.0, -3.0], [1.0, 1.0, 1.0])
    assert abs(s - 480 / (1.2 * 4.0)) < 1e-12 and (X0, Y0, cx, cy) == (0.0, 0.5, 320.0, 240.0)


def test_oracle_placement_is_the_reference_recorded():
    """tests/skeleton_ref.place / numpy slicing against the reference's recorded resize_or_crop / crop_bottom on every branch."""
    g = load("g30_motion_video")
    n_resize = len([k for k in g.files if k.startswith("resize/") and k.endswith("/in")])
    assert n_resize >= 8
    seen = set()
    for k in range(n_resize):
        img, (w, h), out = g[f"resize/{k}/in"], g[f"resize/{k}/wh"], g[f"resize/{k}/out"]
        seen.add((np.sign(img.shape[1] - w), np.sign(img.shape[0] - h)))
        assert np.array_equal(skeleton_ref.place(img, int(w), int(h)), out), k
    assert seen == {(1, 1), (1, -1), (1, 0), (-1, 0), (0, 1), (0, -1), (0, 0)}   # every branch the reference can execute
    k = 0
    while f"crop/{k}/in" in g.files:
        img, n = g[f"crop/{k}/in"], int(g[f"crop/{k}/n"])
        assert np.array_equal(img[:img.shape[0] - n], g[f"crop/{k}/out"])
        k += 1
    assert k >= 3


def test_depth_keys_of_the_drawn_seeds_are_apart():
    """The per-frame order is the one discrete decision of dposer_draw_skeletons: for the seeds test_gpu_draw.py draws, the oracle's
    smallest gap between two depth keys of a frame exceeds 1e-4 (fp32 keys of values below 16 carry errors under 2e-6)."""
    from dposer_amd.body_model.utils import get_smpl_skeleton
    bones = get_smpl_skeleton()
    for frames, seeds in SEQUENCE_SEEDS.items():
        for seed in seeds:
            seq = skeleton_ref.random_sequence(seed, frames)
            assert np.abs(seq[..., 2]).max() < 16.0
            gap = skeleton_ref.min_key_gap(seq, bones)
            print(f"frames {frames} seed {seed}: min key gap {gap:.3e}")
            assert gap > KEY_GAP, (frames, seed, gap)


def test_oracle_draws_the_hand_cases():
    """The oracle itself on cases worked by hand: a horizontal bone of width 2 through pixel centres, a disc at a pixel centre."""
    j = np.array([[[2.5, 3.5, 0.0], [7.5, 3.5, 0.0]]], np.float32)
    view = (1.0, 0.0, 0.0, 0.0, 0.0)
    red = np.array([[255, 0, 0]], np.uint8)
    black = np.zeros((2, 3), np.uint8)
    img, _ = skeleton_ref.draw_skeletons(j, [[0, 1]], red, black, view, (8, 12), line_width=2.0, joint_radius=0.0, y_up=False,
                                         background_color=(255, 255, 255), visible=None)
    img = img[0]
    # joint_radius 0: coverage clamp(0.5 - d) is 0.5 at the centre the disc sits on; bones first, so a black half-disc on top of the ends
    assert tuple(img[3, 4]) == (255, 0, 0) and tuple(img[2, 4]) == (255, 128, 128) and tuple(img[1, 4]) == (255, 255, 255)
    assert tuple(img[3, 2]) == (128, 0, 0)                                         # red, then half black
    assert tuple(img[3, 1]) == (255, 128, 128) and tuple(img[3, 0]) == (255, 255, 255)   # the cap: d = 1 -> a = 0.5; d = 2 -> 0
