"""The skeleton rasteriser and the panel compositor on the GPU (dposer_draw_skeletons, dposer_compose_panels, csrc/draw.hip) against the
fp64 oracle of tests/skeleton_ref.py, and the host API built on them: vis_skeletons, the motion-video functions,
MotionDenoise.optimize(vis=True) and generation_process.

Tolerances.  Apart from the per-frame paint order, a drawn pixel is a continuous function of the inputs, and the fp32 error of a coverage
(screen coordinates of a few hundred pixels: 1e-4 at most) is orders below 1 / 255: only the final rounding can flip, so every pixel
must lie within 1 level of the oracle and none is exempt.  The paint order is discrete; tests/test_draw_cpu.py asserts that the seeds
drawn here keep the depth keys of a frame more than 1e-4 apart.  Everything in the compositor except the bilinear tap is a byte move
and must be exact; the tap is held to 1 level for the same reason as above."""
import os

import numpy as np
import pytest
import torch

import skeleton_ref
from gpu_common import make_model
from helpers import load
from test_draw_cpu import SEQUENCE_SEEDS

DEV = "cuda:0"
pytestmark = pytest.mark.gpu


def _bones():
    from dposer_amd.body_model.utils import get_smpl_skeleton
    return get_smpl_skeleton()


def _draw(joints, bones, hw, view, **kw):
    from dposer_amd.body_model.visual import draw_skeletons
    return draw_skeletons(torch.as_tensor(np.asarray(joints, np.float32), device=DEV), bones, hw, view, **kw).cpu().numpy()


def _max_diff(a, b):
    return int(np.abs(a.astype(np.int16) - b.astype(np.int16)).max())


RED = np.array([[255, 0, 0]], np.uint8)
UNIT_VIEW = (1.0, 0.0, 0.0, 0.0, 0.0)              # screen = joint coordinates with y_up = False


def test_hand_cases_are_exact():
    """An axis-aligned bone of width 2 through pixel centres and a disc of radius 2 at a pixel centre: every coverage is a multiple of
    1 / 2 or decided by a distance that fp32 holds exactly, so the bytes are the hand-computed ones and the oracle's."""
    j = np.array([[[2.5, 3.5, 0.0], [7.5, 3.5, 0.0]]], np.float32)
    black2 = np.zeros((2, 3), np.uint8)
    kw = dict(bone_color=RED, joint_color=black2, line_width=2.0, joint_radius=0.0, y_up=False)
    for hw in ((8, 12), (8, 11)):                                                  # the dword path and the byte path
        img = _draw(j, [[0, 1]], hw, UNIT_VIEW, **kw)[0]
        ref, _ = skeleton_ref.draw_skeletons(j, [[0, 1]], RED, black2, UNIT_VIEW, hw, line_width=2.0, joint_radius=0.0, y_up=False)
        assert np.array_equal(img, ref[0])
        assert tuple(img[3, 4]) == (255, 0, 0) and tuple(img[2, 4]) == (255, 128, 128) and tuple(img[1, 4]) == (255, 255, 255)
        assert tuple(img[3, 2]) == (128, 0, 0) and tuple(img[3, 1]) == (255, 128, 128) and tuple(img[3, 0]) == (255, 255, 255)
        assert tuple(img[4, 7]) == (255, 128, 128) and tuple(img[5, 7]) == (255, 255, 255)
    # a disc alone: radius 2 at the centre of pixel (row 5, col 6) over a black background
    d = np.array([[[6.5, 5.5, 0.0]]], np.float32)
    blue = np.array([[0, 0, 255]], np.uint8)
    img = _draw(d, np.zeros((0, 2), np.int64), (12, 16), UNIT_VIEW, joint_color=blue, joint_radius=2.0, y_up=False, background_color=(0, 0, 0))[0]
    assert tuple(img[5, 6]) == (0, 0, 255) and tuple(img[5, 8]) == (0, 0, 128) and tuple(img[5, 9]) == (0, 0, 0)      # d = 0, 2, 3
    assert tuple(img[3, 6]) == (0, 0, 128) and tuple(img[5, 7]) == (0, 0, 255) and tuple(img[2, 6]) == (0, 0, 0)
    ref, _ = skeleton_ref.draw_skeletons(d, np.zeros((0, 2), int), None, blue, UNIT_VIEW, (12, 16), joint_radius=2.0, y_up=False,
                                         background_color=(0, 0, 0))
    assert _max_diff(img, ref[0]) <= 1 and np.array_equal(img[5], ref[0][5]) and np.array_equal(img[:, 6], ref[0][:, 6])
    # y_up flips the rows about cy, the view scales and shifts
    up = _draw(j, [[0, 1]], (8, 12), (1.0, 0.0, 0.0, 0.0, 8.0), **dict(kw, y_up=True))[0]
    assert tuple(up[4, 4]) == (255, 0, 0) and tuple(up[5, 4]) == (255, 128, 128)   # screen y = 8 - 3.5 = 4.5
    sc = _draw(j, [[0, 1]], (16, 24), (2.0, 0.25, 0.25, 0.0, 0.0), **kw)[0]          # screen = 2 (X - 0.25): (4.5, 6.5) - (14.5, 6.5)
    assert tuple(sc[6, 9]) == (255, 0, 0) and tuple(sc[6, 4]) == (128, 0, 0) and tuple(sc[6, 3]) == (255, 128, 128)


def test_near_bone_beats_far_bone_and_dropped_joints_vanish():
    j = np.array([[[2.5, 8.5, 0.0], [14.5, 8.5, 0.0], [8.5, 2.5, 1.0], [8.5, 14.5, 1.0]]], np.float32)   # horizontal at z 0, vertical at z 1
    cols = np.array([[255, 0, 0], [0, 0, 255]], np.uint8)
    none = np.zeros((4, 3), np.uint8)
    kw = dict(joint_color=none, line_width=2.0, joint_radius=0.0, y_up=False)
    for bones, colors in (([[0, 1], [2, 3]], cols), ([[2, 3], [0, 1]], cols[::-1].copy())):      # both list orders
        near_v = _draw(j, bones, (18, 18), UNIT_VIEW, bone_color=colors, z_toward_viewer=True, **kw)[0]      # larger z nearer: the vertical bone
        near_h = _draw(j, bones, (18, 18), UNIT_VIEW, bone_color=colors, z_toward_viewer=False, **kw)[0]
        assert tuple(near_v[8, 8]) == (0, 0, 255) and tuple(near_h[8, 8]) == (255, 0, 0)
        assert tuple(near_v[8, 5]) == (255, 0, 0) and tuple(near_v[5, 8]) == (0, 0, 255)
        for zt in (True, False):
            ref, _ = skeleton_ref.draw_skeletons(j, bones, colors, none, UNIT_VIEW, (18, 18), line_width=2.0, joint_radius=0.0, y_up=False,
                                                 z_toward_viewer=zt)
            assert np.array_equal(_draw(j, bones, (18, 18), UNIT_VIEW, bone_color=colors, z_toward_viewer=zt, **kw)[0], ref[0])
    # an invisible or NaN joint removes its bones and its disc; the other bone stays
    grey = np.full((4, 3), 90, np.uint8)
    kw = dict(bone_color=cols, joint_color=grey, line_width=2.0, joint_radius=2.0, y_up=False)
    full = _draw(j, [[0, 1], [2, 3]], (18, 18), UNIT_VIEW, **kw)[0]
    only_h = _draw(j[:, :2], [[0, 1]], (18, 18), UNIT_VIEW, **dict(kw, bone_color=cols[:1], joint_color=grey[:2]))[0]
    inv = _draw(j, [[0, 1], [2, 3]], (18, 18), UNIT_VIEW, visible=[1, 1, 0, 1], **kw)[0]
    jn = j.copy()
    jn[0, 2, 1] = np.nan
    nan = _draw(jn, [[0, 1], [2, 3]], (18, 18), UNIT_VIEW, **kw)[0]
    assert not np.array_equal(full, only_h)
    for got in (inv, nan):
        # joint 3's disc is still drawn (it is visible and finite)
        ref, _ = skeleton_ref.draw_skeletons(j, [[0, 1], [2, 3]], cols, grey, UNIT_VIEW, (18, 18), visible=[1, 1, 0, 1], line_width=2.0,
                                             joint_radius=2.0, y_up=False)
        assert _max_diff(got, ref[0]) <= 1
        assert np.array_equal(got[:11], only_h[:11])                                # rows away from joint 3's disc: the vertical bone is gone
    jinf = j.copy()
    jinf[0, 0, 0] = np.inf
    assert np.array_equal(_draw(jinf, [[0, 1], [2, 3]], (18, 18), UNIT_VIEW, visible=[1, 0, 1, 1], **kw)[0],
                          _draw(j, [[0, 1], [2, 3]], (18, 18), UNIT_VIEW, visible=[0, 0, 1, 1], **kw)[0])


@pytest.mark.parametrize("frames", [1, 60])
@pytest.mark.parametrize("hw", [(480, 640), (37, 53)])
def test_random_sequences_within_one_level_everywhere(frames, hw):
    from dposer_amd.body_model import visual
    bones = _bones()
    bcol = visual.rainbow_swapped(len(bones))
    jcol = visual.skeleton_joint_colors(bones, bcol, 22)
    for seed in SEQUENCE_SEEDS[frames]:
        seq = skeleton_ref.random_sequence(seed, frames)
        lo, hi = seq.reshape(-1, 3).min(0), seq.reshape(-1, 3).max(0)
        view = visual.skeleton_view([lo[0], lo[1], 0.0], [hi[0], hi[1], 0.0], hw)     # fit x and y: the skeleton fills the canvas
        rs = np.random.RandomState(seed)
        bg = rs.randint(0, 256, (frames,) + hw + (3,)).astype(np.uint8) if seed % 2 else None
        lw, jr = (visual.LINE_WIDTH_PX, visual.JOINT_RADIUS_PX) if hw[0] > 100 else (1.3, 1.9)
        got = _draw(seq, bones, hw, view, line_width=lw, joint_radius=jr, background=bg)
        ref, _ = skeleton_ref.draw_skeletons(seq, bones, bcol, jcol, view, hw, line_width=lw, joint_radius=jr, background=bg)
        diff = np.abs(got.astype(np.int16) - ref.astype(np.int16))
        drawn = (ref != (255 if bg is None else bg)).any(axis=-1).mean()
        print(f"frames {frames} {hw} seed {seed}: max diff {diff.max()}, pixels off by one {(diff.max(axis=-1) == 1).mean():.2e}, drawn {drawn:.3f}")
        assert drawn > 0.01                                                         # the skeleton is on the canvas
        assert diff.max() <= 1
        # the automatic view is skeleton_view of the batch's bounds (all three axes)
        if bg is None and frames == 1:
            assert np.array_equal(_draw(seq, bones, hw, None, line_width=lw, joint_radius=jr),
                                  _draw(seq, bones, hw, visual.skeleton_view(lo, hi, hw), line_width=lw, joint_radius=jr))


def test_two_calls_are_bit_identical():
    bones = _bones()
    seq = skeleton_ref.random_sequence(SEQUENCE_SEEDS[60][0], 60)
    a = _draw(seq, bones, (480, 640), None)
    b = _draw(seq, bones, (480, 640), None)
    assert np.array_equal(a, b)


def test_output_beyond_two_gib_last_frame():
    """2331 frames of 640 x 480 x 3 bytes pass 2^31: the last frame equals that frame drawn alone (64-bit addressing)."""
    from dposer_amd.body_model.visual import draw_skeletons, skeleton_view
    bones = _bones()
    B = 2331
    assert B * 480 * 640 * 3 > 2 ** 31
    seq = skeleton_ref.random_sequence(5, 37)
    seq = np.concatenate([seq] * (B // 37 + 1))[:B].copy()
    seq[-1] = skeleton_ref.random_sequence(6, 1)[0] * np.float32(0.9)
    view = skeleton_view(seq.reshape(-1, 3).min(0), seq.reshape(-1, 3).max(0))
    j = torch.as_tensor(seq, device=DEV)
    big = draw_skeletons(j, bones, view=view)
    assert big.numel() > 2 ** 31
    alone = draw_skeletons(j[-1:], bones, view=view)
    assert torch.equal(big[-1], alone[0]) and torch.equal(big[0], draw_skeletons(j[:1], bones, view=view)[0])
    assert bool((alone[0] != 255).any())


# ---- compositor ----------------------------------------------------------------------------------------------------------------------
def _compose(panels, n, out_hw, **kw):
    from dposer_amd.utils.motion_video import compose_panels
    dev = [dict(p, src=torch.as_tensor(np.ascontiguousarray(p["src"]), device=DEV)) for p in panels]
    return compose_panels(dev, n, out_hw, **kw).cpu().numpy()


def test_compositor_byte_moves_are_exact():
    rs = np.random.RandomState(11)
    img = lambda n, h, w: rs.randint(0, 256, (n, h, w, 3)).astype(np.uint8)
    N = 3
    strip = img(1, 5, 16)[0]
    for out_w in (48, 45):                                                           # dword stores / byte stores
        panels = [
            dict(src=img(N, 30, 23), crop=(3, 2, 19, 25), cell=(20, 16), strip=strip, x=0, fill=(9, 8, 7)),      # wider + taller: centre, bottom
            dict(src=img(1, 12, 9), cell=(20, 14), x=16, fill=(200, 100, 50)),                                    # shared source; narrower + shorter
            dict(src=img(N, 20, 40), crop=(1, 0, 33, 20), cell=(20, 12), strip=img(1, 3, 12)[0], x=31),          # wider, same height
        ]
        got = _compose(panels, N, (27, out_w), out_fill=(1, 2, 3))
        assert np.array_equal(got, skeleton_ref.compose(panels, N, (27, out_w), out_fill=(1, 2, 3)))
        assert tuple(got[0, 26, out_w - 1]) == (1, 2, 3) and tuple(got[1, 26, 2]) == (1, 2, 3)                   # below a strip / beside the panels


def test_compositor_reproduces_the_reference_goldens():
    """resize_or_crop / crop_bottom of the reference, recorded on every branch it can execute, through the product's functions."""
    from dposer_amd.utils.motion_video import crop_bottom, resize_or_crop
    g = load("g30_motion_video")
    k = 0
    while f"resize/{k}/in" in g.files:
        w, h = (int(v) for v in g[f"resize/{k}/wh"])
        out = resize_or_crop(g[f"resize/{k}/in"], w, h)
        assert isinstance(out, np.ndarray) and out.dtype == np.uint8 and np.array_equal(out, g[f"resize/{k}/out"]), k
        k += 1
    assert k >= 8
    k = 0
    while f"crop/{k}/in" in g.files:
        assert np.array_equal(crop_bottom(g[f"crop/{k}/in"], int(g[f"crop/{k}/n"])), g[f"crop/{k}/out"]), k
        k += 1
    assert k >= 3
    # the case the reference cannot execute: narrower and taller, each axis on its own
    img = np.random.RandomState(2).randint(0, 256, (40, 10, 3)).astype(np.uint8)
    assert np.array_equal(resize_or_crop(img, 24, 30), skeleton_ref.place(img, 24, 30))


def test_bilinear_resize_within_one_level():
    rs = np.random.RandomState(12)
    for (h, w), (hr, wr) in (((48, 64), (43, 57)), ((20, 31), (47, 80)), ((37, 53), (37, 21)), ((480, 640), (432, 576))):
        src = rs.randint(0, 256, (2, h, w, 3)).astype(np.uint8)
        got = _compose([dict(src=src, resize=(hr, wr), cell=(hr, wr))], 2, (hr, wr))
        for n in range(2):
            ref, exact = skeleton_ref.resize_bilinear(src[n], hr, wr)
            diff = np.abs(got[n].astype(np.int16) - ref.astype(np.int16))
            assert diff.max() <= 1, ((h, w), (hr, wr))
            assert np.abs(got[n] - exact).max() <= 0.5 + 1e-2                        # a flip only where the exact value sits on a boundary
    # a constant image stays constant, an identity resize is a byte move
    flat = np.full((1, 9, 11, 3), 77, np.uint8)
    assert (_compose([dict(src=flat, resize=(20, 5), cell=(20, 5))], 1, (20, 5)) == 77).all()


def test_compose_motion_frames_layout():
    from dposer_amd.utils import motion_video as mv
    rs = np.random.RandomState(13)
    N = 4
    sk = rs.randint(0, 256, (N, 480, 640, 3)).astype(np.uint8)
    ou = rs.randint(0, 256, (N, 512, 384, 3)).astype(np.uint8)
    gt = rs.randint(0, 256, (N, 512, 384, 3)).astype(np.uint8)
    t = lambda a: torch.as_tensor(a, device=DEV)
    got = mv.compose_motion_frames(t(sk), t(ou), t(gt))
    assert got.is_cuda and tuple(got.shape) == (N, 430, 768, 3) and got.dtype == torch.uint8
    got = got.cpu().numpy()
    titles = [mv.title_strip(s) for s in ("Noisy Joints", "DPoser(Ours)", "GT")]
    for n in range(N):
        joint = skeleton_ref.place(skeleton_ref.resize_bilinear(sk[n], 432, 576)[0], 256, 400)      # process_joint
        assert _max_diff(got[n, :400, :256], joint) <= 1
        assert np.array_equal(got[n, :400, 256:512], skeleton_ref.place(ou[n][:492], 256, 400))     # process_body: crop_bottom 20
        assert np.array_equal(got[n, :400, 512:], skeleton_ref.place(gt[n][:492], 256, 400))
        for k in range(3):
            assert np.array_equal(got[n, 400:, 256 * k:256 * (k + 1)], titles[k])
    assert (titles[0] == 255).mean() > 0.8 and titles[0].shape == (30, 256, 3)


# ---- host API ------------------------------------------------------------------------------------------------------------------------
def test_vis_skeletons_outputs(tmp_path):
    import render_ref
    from dposer_amd.body_model.visual import vis_skeletons
    from dposer_amd.utils.motion_video import read_video
    seq = skeleton_ref.random_sequence(3, 7, spread=(0.35, 0.5, 0.3))
    out_dir = str(tmp_path / "renders")
    vis_skeletons(seq, out_dir)
    names = sorted(os.listdir(out_dir))
    assert names == [f"frame_{i:04d}.png" for i in range(7)]
    frames = np.stack([render_ref.decode_png(open(os.path.join(out_dir, n), "rb").read()) for n in names])
    assert frames.shape == (7, 480, 640, 3)
    assert (frames[0, 0, 0] == 255).all() and 0.002 < (frames != 255).any(axis=-1).mean() < 0.2
    # upright: the joint with the largest y is drawn highest (smallest row); larger x further right
    ys, xs = np.nonzero((frames[0] != 255).any(axis=-1))
    top, bottom = seq[0, :, 1].argmax(), seq[0, :, 1].argmin()
    assert seq[0, top, 1] - seq[0, bottom, 1] > 0.2 and ys.min() < 240 < ys.max() and xs.min() < 320 < xs.max()
    from dposer_amd.body_model import visual
    lo, hi = seq.reshape(-1, 3).min(0), seq.reshape(-1, 3).max(0)
    s, X0, Y0, cx, cy = visual.skeleton_view(lo, hi)
    assert abs(ys.min() - (cy - s * (seq[0, top, 1] - Y0))) < 8 and abs(ys.max() - (cy - s * (seq[0, bottom, 1] - Y0))) < 8
    vis_skeletons(seq, str(tmp_path / "clip.mp4"))
    assert sorted(os.listdir(tmp_path)) == ["clip.avi", "renders"]
    video, fps = read_video(str(tmp_path / "clip.avi"))
    assert fps == 20.0 and np.array_equal(video, frames)
    with pytest.raises(ValueError):
        vis_skeletons(seq, str(tmp_path / "clip.gif"))
    vis_skeletons(seq[0], str(tmp_path / "one.png"))                                 # a single frame: its own bounds
    one = render_ref.decode_png(open(str(tmp_path / "one.png"), "rb").read())
    assert one.shape == (480, 640, 3) and (one != 255).any()


def _motion_denoise(out_path):
    from dposer_amd.body_model.body_model import BodyModel
    from dposer_amd.body_model.synthetic import make_synthetic_smplx_asset
    from dposer_amd.dataset.AMASS import Posenormalizer
    from dposer_amd.tasks.motion_denoising import MotionDenoise
    from oracle import fk_ref
    cfg, m, p = make_model(63, precision="fp32")
    asset = make_synthetic_smplx_asset(seed=0)
    bm = BodyModel(asset).to(DEV)
    g = load("g10_normalizer")
    stats = {k.split("/")[-1]: torch.tensor(g[k]) for k in g.files if k.startswith("stats/axis_normalize")}
    T, iters, spi = 12, 1, 3
    gt = g["raw"][:T].astype(np.float32)
    rs = np.random.RandomState(7)
    init = (gt + rs.standard_normal(gt.shape) * 0.05).astype(np.float32)
    _, jgt, _, _ = fk_ref.smplx_forward(asset, gt.astype(np.float64), dtype=np.float64)
    joints3d = (jgt[:, :22] + rs.standard_normal((T, 22, 3)) * 0.04).astype(np.float32)
    noise = rs.standard_normal((iters * spi, T, 63)).astype(np.float32)

    class Args:
        device = DEV

    nz = Posenormalizer(stats, device=DEV, normalize=True, min_max=False, rot_rep="axis")
    md = MotionDenoise(cfg, Args(), m, bm, sde_N=500, batch_size=T, normalizer=nz, out_path=out_path)
    dev = lambda a: torch.tensor(a, device=DEV)
    run = lambda vis: md.optimize(dev(joints3d), gt_poses=dev(gt), time_strategy="3", iterations=iters, steps_per_iter=spi, noise=dev(noise),
                                  init_poses=dev(init), vis=vis)
    return run, T


def test_motion_denoise_vis_writes_the_video_and_keeps_the_metrics(tmp_path):
    from dposer_amd.utils.motion_video import read_video
    out = str(tmp_path / "md")
    run, T = _motion_denoise(out)
    plain = run(False)
    assert not os.path.exists(out)
    shown = run(True)
    for k in ("init_MPJPE", "MPJPE", "MPVPE", "pose_body"):
        assert torch.equal(torch.as_tensor(plain[k]), torch.as_tensor(shown[k])), k
    renders = sorted(os.listdir(os.path.join(out, "renders")))
    assert renders == sorted(f"{stem}_{i:04d}.png" for stem in ("frame", "gt", "out") for i in range(T))
    assert sorted(os.listdir(os.path.join(out, "merges"))) == [f"merge_{i:04d}.png" for i in range(T)]
    video, fps = read_video(os.path.join(out, "motion.avi"))
    assert video.shape == (T, 430, 768, 3) and fps == 20.0
    import render_ref
    merged = render_ref.decode_png(open(os.path.join(out, "merges", "merge_0003.png"), "rb").read())
    assert np.array_equal(video[3], merged)
    gt3 = render_ref.decode_png(open(os.path.join(out, "renders", "gt_0003.png"), "rb").read())
    assert gt3.shape == (512, 384, 3) and (gt3 != 255).any() and np.array_equal(merged[:400, 512:], skeleton_ref.place(gt3[:492], 256, 400))
    for x0 in (0, 256, 512):
        assert (merged[:400, x0:x0 + 256] != 255).any()                              # every panel shows something


def test_generation_process_writes_the_videos(tmp_path):
    from dposer_amd.algorithms.advanced import sde_lib
    from dposer_amd.body_model.body_model import BodyModel
    from dposer_amd.body_model.synthetic import make_synthetic_smplx_asset
    from dposer_amd.dataset.AMASS import Posenormalizer
    from dposer_amd.tasks.generation import generation_process
    from dposer_amd.utils.motion_video import read_video
    cfg, m, p = make_model(63, precision="fp32")
    bm = BodyModel(make_synthetic_smplx_asset(seed=0)).to(DEV)
    g = load("g10_normalizer")
    stats = {k.split("/")[-1]: torch.tensor(g[k]) for k in g.files if k.startswith("stats/axis_normalize")}
    nz = Posenormalizer(stats, device=DEV, normalize=True, min_max=False, rot_rep="axis")
    sde = sde_lib.subVPSDE(beta_min=cfg.model.beta_min, beta_max=cfg.model.beta_max, N=1000)
    torch.manual_seed(0)
    paths = generation_process(m, sde, cfg, nz, bm, str(tmp_path / "generation_process"), video_num=2)
    assert [os.path.basename(q) for q in paths] == ["generation_process0.avi", "generation_process1.avi"]
    assert sorted(os.listdir(tmp_path / "generation_process")) == ["generation_process0.avi", "generation_process1.avi"]
    clips = []
    for q in paths:
        video, fps = read_video(q)
        assert video.shape == (100, 512, 384, 3) and fps == 30.0
        assert (video[-1] != 255).any() and (video[-1, 0, 0] == 255).all()            # a body over the white canvas
        clips.append(video)
    assert not np.array_equal(clips[0][-1], clips[1][-1])
