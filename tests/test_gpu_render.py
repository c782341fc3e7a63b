"""The mesh renderer on the GPU (dposer_render_meshes, csrc/render.hip) against the fp64 oracle of tests/render_ref.py: hand cases bit for
bit, closed body-sized tori (flat and smooth) on every pixel the oracle decides, several meshes per image, triangles around the tile and
large-list thresholds, invariance under face permutation / grouping / repetition, the synthetic SMPL-X asset, 64-bit addressing, and the
reference's host API (render_mesh, multiple_render as demo.py calls it, Renderer)."""
import os

import numpy as np
import pytest
import torch

import render_ref
import si_ref

DEV = "cuda:0"
pytestmark = pytest.mark.gpu

FOCAL, PRINCPT = (1500.0, 1500.0), (200.0, 192.0)


def _render(v, f, K, hw, **kw):
    from dposer_amd.body_model.visual import render_meshes
    t = lambda a: a if a is None or torch.is_tensor(a) else torch.as_tensor(np.asarray(a), device=DEV)
    for k in ("transforms", "image_of_mesh", "base_color"):
        if k in kw and kw[k] is not None and not isinstance(kw[k], tuple):
            kw[k] = t(kw[k])
    out = render_meshes(torch.as_tensor(np.asarray(v, np.float32), device=DEV), torch.as_tensor(np.asarray(f), device=DEV), t(np.asarray(K, np.float32)),
                        hw, **kw)
    return {k: x.cpu().numpy() for k, x in out.items()}


def _oracle_kw(kw):
    keep = ("transforms", "image_of_mesh", "base_color", "lights", "ambient", "smooth", "znear", "zfar")
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in kw.items() if k in keep}


def _check(got, ref, rgb_tol=1.0, name=""):
    amb = ref["ambiguous"]
    ok = ~amb
    bad = (got["face_id"] != ref["face_id"]) & ok
    assert not bad.any(), (name, np.argwhere(bad)[:10], got["face_id"][bad][:10], ref["face_id"][bad][:10])
    assert np.array_equal(got["mesh_id"][ok], ref["mesh_id"][ok]), name
    cov = ref["covered"] & ok
    assert np.array_equal(got["depth"][~ref["covered"] & ok], np.zeros(int((~ref["covered"] & ok).sum()), np.float32))
    rel = np.abs(got["depth"][cov] - ref["depth"][cov]) / ref["depth"][cov]
    assert rel.max() < 1e-5, (name, rel.max())
    d = np.abs(got["rgb"][cov].astype(np.float64) - ref["rgb255"][cov])
    assert d.max() <= rgb_tol + 1e-6 + 0.5, (name, d.max())        # rint of 255 c: +-0.5, plus the fp32 shading
    assert amb.mean() < 0.02, (name, amb.mean())
    return cov.sum()


def _flat(v):
    """screen = model coordinates: identity transform, fx = fy = 1, c = 0, z = 1 (every edge value exact in fp32)."""
    return np.asarray(v, np.float32)


K1 = [1.0, 1.0, 0.0, 0.0]


# ---- 1. hand cases ---------------------------------------------------------------------------------------------------------------------
def test_one_triangle_and_the_shared_diagonal():
    sq = _flat([[1.5, 1.5, 1], [7.5, 1.5, 1], [7.5, 7.5, 1], [1.5, 7.5, 1]])
    for faces in ([[0, 1, 2]], [[0, 1, 2], [0, 2, 3]], [[2, 1, 0], [0, 3, 2]]):
        got = _render(sq[None], faces, K1, (10, 10))
        ref = render_ref.render(sq[None], faces, K1, 10, 10)
        assert np.array_equal(got["face_id"], ref["face_id"]) and np.array_equal(got["mesh_id"], ref["mesh_id"])
        if len(faces) == 2:                                  # no hole, nothing twice: the 6 x 6 block of centres, top-left rule
            want = np.full((10, 10), False)
            want[1:7, 1:7] = True
            assert np.array_equal(got["face_id"][0] >= 0, want)
    assert (got["depth"][0][got["face_id"][0] >= 0] == 1.0).all()


@pytest.mark.parametrize("order", [0, 1])
def test_nearer_triangle_wins_in_both_face_orders(order):
    a = [[2 * x, 2 * y, 2.0] for x, y in ((1, 1), (9, 1), (1, 9))]          # z = 2
    b = [[3 * x, 3 * y, 3.0] for x, y in ((0.5, 0.5), (9.5, 0.5), (0.5, 9.5))]   # z = 3, the same region on screen
    v = _flat(a + b)
    faces = [[0, 1, 2], [3, 4, 5]] if order == 0 else [[3, 4, 5], [0, 1, 2]]
    got = _render(v[None], faces, K1, (12, 12))
    near = 0 if order == 0 else 1
    both = (got["face_id"][0] >= 0)
    a_cov = render_ref.render(v[None], [faces[near]], K1, 12, 12)["covered"][0]
    assert (got["face_id"][0][a_cov] == near).all() and (both & ~a_cov).any()


def test_interpenetrating_triangles_switch_inside_a_row():
    # A tilts from z = 2 (left) to z = 4 (right), 1 / z linear on screen; B is flat at z = 3: they cross at x = 20 / 3
    za = lambda x: 2 + 2 * x / 10
    A = [[x * za(x), y * za(x), za(x)] for x, y in ((0, 0), (10, 0), (0, 10), (10, 10))]
    Bq = [[x * 3, y * 3, 3.0] for x, y in ((0.25, 0.25), (9.75, 0.25), (0.25, 9.75), (9.75, 9.75))]
    v = _flat(A + Bq)
    f = [[0, 1, 3], [0, 3, 2], [4, 5, 7], [4, 7, 6]]
    got = _render(v[None], f, K1, (10, 10))
    ref = render_ref.render(v[None], f, K1, 10, 10)
    ok = ~ref["ambiguous"]
    assert np.array_equal(got["face_id"][ok], ref["face_id"][ok])
    row = got["face_id"][0, 5]
    assert set(row[1:6]) <= {0, 1} and set(row[7:10]) <= {2, 3}


def test_dropped_triangles_write_nothing():
    v = _flat([[1, 1, 0.005], [8, 1, 0.005], [1, 8, 0.005],          # behind znear
               [1, 1, 1], [4, 4, 1], [7, 7, 1],                       # zero area
               [1, 1, 1], [8, 1, 1], [np.nan, 8, 1]])                 # a NaN corner
    got = _render(v[None], [[0, 1, 2], [3, 4, 5], [6, 7, 8]], [1, 1, 0, 0], (10, 10), background_color=(7, 8, 9), znear=0.01)
    assert (got["face_id"] == -1).all() and (got["mesh_id"] == -1).all() and (got["depth"] == 0).all()
    assert (got["rgb"] == np.array([7, 8, 9], np.uint8)).all()


def test_exact_depth_ties_go_to_the_lower_mesh_and_face():
    t = [[1, 1, 2], [9, 1, 2], [1, 9, 2]]
    v = _flat(t + t)                                                  # two faces with the same corners, different indices
    for faces, want in (([[0, 1, 2], [3, 4, 5]], 0), ([[3, 4, 5], [0, 1, 2]], 0), ([[4, 5, 3], [2, 0, 1]], 0)):
        got = _render(v[None] * [2, 2, 1], faces, [2, 2, 0, 0], (10, 10))
        cov = got["face_id"][0] >= 0
        assert cov.sum() > 10 and (got["face_id"][0][cov] == want).all()
    V2 = np.stack([v, v]) * [2, 2, 1]
    got = _render(V2, [[0, 1, 2]], [2, 2, 0, 0], (10, 10), image_of_mesh=np.array([0, 0], np.int32))
    cov = got["mesh_id"][0] >= 0
    assert (got["mesh_id"][0][cov] == 0).all()


# ---- 2. closed tori ------------------------------------------------------------------------------------------------------------------
def _torus_scene(views, seed=3):
    from dposer_amd.body_model import visual
    X, F = render_ref.body_torus(seed=seed)
    c = X.astype(np.float64).mean(0)
    T = np.stack([visual.render_mesh_transform(c, *visual.parse_view(vw)) for vw in views]).astype(np.float32)
    return X, F, T


LIGHTS = [(0, 0.0, 0.0, -1.0, 0.25, 0.25, 0.25), (0, 0.3, -0.5, -0.8, 0.3, 0.2, 0.1), (1, 1.0, -1.0, -2.0, 0.2, 0.3, 0.4)]


@pytest.mark.parametrize("smooth", [False, True])
@pytest.mark.parametrize("hw,scale", [((64, 96), 0.2), ((160, 200), 0.45), ((384, 512), 1.0)])
def test_torus_matches_the_oracle(hw, scale, smooth):
    views = ["front", "half_left_above", "back_bottom", "right"]
    X, F, T = _torus_scene(views)
    V = np.stack([X] * len(views))
    K = np.array([[FOCAL[0] * scale, FOCAL[1] * scale, hw[1] / 2, hw[0] / 2]] * len(views), np.float32)
    kw = dict(transforms=T, base_color=(0.93, 0.6, 0.4), lights=LIGHTS, ambient=0.2, smooth=smooth)
    got = _render(V, F, K, hw, **kw)
    ref = render_ref.render(V, F, K, hw[0], hw[1], **_oracle_kw(kw))
    n = _check(got, ref, name=f"{hw} smooth={smooth}")
    assert n > 0.05 * hw[0] * hw[1] * len(views)


def test_several_meshes_per_image():
    X, F, _ = _torus_scene(["front"])
    V = np.stack([si_ref.smooth_deform(X, 10 + k) for k in range(5)])
    T = np.zeros((5, 3, 4), np.float32)
    T[:, :, :3] = np.eye(3)
    T[:, :, 3] = [[-0.5, 0, 6], [0.5, 0.1, 6.2], [0, 0, 5], [0.3, -0.2, 6], [0, 0, 7]]
    T[:, 1, 1] = -1
    img = np.array([0, 0, 1, 1, 1], np.int32)
    K = np.array([[400, 400, 96, 64], [380, 390, 90, 70]], np.float32)
    col = np.random.RandomState(0).uniform(0.2, 1, (5, 3)).astype(np.float32)
    kw = dict(transforms=T, image_of_mesh=img, base_color=col, lights=LIGHTS, ambient=0.1)
    got = _render(V, F, K, (128, 192), **kw)
    ref = render_ref.render(V, F, K, 128, 192, **_oracle_kw(kw))
    _check(got, ref, name="multi")
    assert set(np.unique(got["mesh_id"][0])) == {-1, 0, 1} and set(np.unique(got["mesh_id"][1])) == {-1, 2, 3, 4}


def _soup(seed, n=600, H=150, W=170):
    """independent triangles of every size from sub-pixel to > 2 tiles, centred on and around tile borders (32 px), random depths."""
    rs = np.random.RandomState(seed)
    size = np.concatenate([rs.uniform(0.5, 4, n // 3), rs.uniform(20, 40, n // 3), rs.uniform(40, 90, n - 2 * (n // 3))])
    cx = np.where(rs.rand(n) < 0.5, 32 * rs.randint(1, 5, n) + rs.uniform(-1, 1, n), rs.uniform(0, W, n))
    cy = np.where(rs.rand(n) < 0.5, 32 * rs.randint(1, 4, n) + rs.uniform(-1, 1, n), rs.uniform(0, H, n))
    z = rs.uniform(2, 6, n)
    corners = rs.uniform(-0.5, 0.5, (n, 3, 2)) * size[:, None, None] + np.stack([cx, cy], -1)[:, None]
    zc = z[:, None] + rs.uniform(-0.3, 0.3, (n, 3))
    v = np.concatenate([corners * zc[..., None] / 100.0, zc[..., None]], -1).reshape(-1, 3)   # projects back with f = 100, c = 0
    return v.astype(np.float32), np.arange(3 * n).reshape(n, 3).astype(np.int32)


def test_triangle_soup_around_tile_borders_and_the_large_list_threshold():
    v, f = _soup(0)
    K = [100.0, 100.0, 0.0, 0.0]
    got = _render(v[None], f, K, (150, 170), lights=LIGHTS, ambient=0.1)
    ref = render_ref.render(v[None], f, K, 150, 170, lights=LIGHTS, ambient=0.1)
    _check(got, ref, name="soup")


# ---- 4. invariance -------------------------------------------------------------------------------------------------------------------
def test_face_permutation_grouping_and_repetition_give_the_same_bits():
    views = ["front", "left", "half_right_above", "back", "bottom", "half_back_bottom", "right_above"]
    X, F, T = _torus_scene(views)
    V = np.stack([si_ref.smooth_deform(X, 40 + k, amp=0.03) for k in range(7)])
    K = np.array([[600, 600, 80, 60]] * 7, np.float32)
    kw = dict(transforms=T, base_color=(0.5, 0.7, 0.9), lights=LIGHTS, ambient=0.1, smooth=True)
    a = _render(V, F, K, (120, 160), **kw)
    b = _render(V, F, K, (120, 160), **kw)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    perm = np.random.RandomState(1).permutation(len(F))
    p = _render(V, F[perm], K, (120, 160), **kw)
    ref = render_ref.render(V, F, K, 120, 160, **_oracle_kw(kw))
    ok = ~ref["ambiguous"]                                                   # (near depth ties are broken by face index)
    mapped = np.where(p["face_id"] >= 0, perm[np.maximum(p["face_id"], 0)], -1)
    assert np.array_equal(mapped[ok], a["face_id"][ok])
    assert np.array_equal(p["depth"][ok], a["depth"][ok]) and np.array_equal(p["rgb"][ok], a["rgb"][ok])
    for n in range(7):
        one = _render(V[n:n + 1], F, K[n:n + 1], (120, 160), **dict(kw, transforms=T[n:n + 1]))
        one["mesh_id"] = np.where(one["mesh_id"] >= 0, one["mesh_id"] + n, -1)                 # (mesh index in the call)
        for k in a:
            assert np.array_equal(one[k][0], a[k][n]), (n, k)


# ---- 5. the synthetic SMPL-X asset (random faces: every face on the large list) ------------------------------------------------------
def test_synthetic_smplx_asset_matches_the_oracle():
    from dposer_amd.body_model.body_model import BodyModel
    from dposer_amd.body_model.synthetic import make_synthetic_smplx_asset
    from dposer_amd.body_model import visual
    bm = BodyModel(make_synthetic_smplx_asset(seed=0)).to(DEV)
    pose = torch.as_tensor(np.random.RandomState(0).standard_normal((2, 63)).astype(np.float32) * 0.3, device=DEV)
    out = bm(pose_body=pose)
    V = out.v.detach().cpu().numpy()
    F = out.f.cpu().numpy()
    T = np.stack([visual.render_mesh_transform(V[b].astype(np.float64).mean(0), *visual.parse_view(vw))
                  for b, vw in enumerate(["front", "half_left_above"])]).astype(np.float32)
    K = np.array([[180, 180, 48, 32]] * 2, np.float32)
    kw = dict(transforms=T, base_color=(0.93, 0.6, 0.4), lights=LIGHTS, ambient=0.3)
    got = _render(V, F, K, (64, 96), **kw)
    ref = render_ref.render(V, F, K, 64, 96, **_oracle_kw(kw))
    _check(got, ref, name="synthetic")
    assert ref["covered"].mean() > 0.2


# ---- 6. addressing past 2^31 ---------------------------------------------------------------------------------------------------------
def test_rgb_output_past_2_31_bytes():
    from dposer_amd.body_model.visual import render_meshes
    N, H, W = 2800, 512, 512                                          # 2.2e9 bytes of rgb
    assert N * H * W * 3 > 2 ** 31
    tri = torch.tensor([[[-0.5, -0.5, 2.0], [0.6, -0.4, 2.5], [-0.2, 0.7, 3.0]]], device=DEV).expand(N, 3, 3).contiguous()
    T = torch.zeros(N, 3, 4, device=DEV)
    T[:, :, :3] = torch.eye(3, device=DEV)
    T[:, 0, 3] = torch.linspace(-0.3, 0.3, N, device=DEV)
    K = torch.tensor([[300.0, 300.0, 256.0, 256.0]], device=DEV).expand(N, 4).contiguous()
    kw = dict(lights=LIGHTS, ambient=0.1, background_color=(1, 2, 3))
    big = render_meshes(tri, torch.tensor([[0, 1, 2]], device=DEV), K, (H, W), transforms=T, outputs=("rgb",), **kw)["rgb"]
    for n in (N - 1, 0):
        one = render_meshes(tri[n:n + 1], torch.tensor([[0, 1, 2]], device=DEV), K[n:n + 1], (H, W), transforms=T[n:n + 1], outputs=("rgb",), **kw)
        assert torch.equal(big[n], one["rgb"][0]), n
    assert (big[N - 1] != big[0]).any()
    del big
    torch.cuda.empty_cache()


def test_vertex_array_past_2_31_elements():
    from dposer_amd.body_model.visual import render_meshes
    B, V = 700, (1 << 20) + 7                                         # 2.2e9 vertex elements
    assert B * V * 3 > 2 ** 31
    v = torch.zeros(B, V, 3, device=DEV)
    v[:, :, 2] = 3.0
    quad = torch.tensor([[-0.4, -0.4, 2.0], [0.5, -0.3, 2.2], [0.4, 0.5, 2.4], [-0.3, 0.4, 2.1]], device=DEV)
    v[:, V - 4:] = quad + torch.linspace(0, 0.2, B, device=DEV)[:, None, None]
    f = torch.tensor([[V - 4, V - 3, V - 2], [V - 4, V - 2, V - 1]], device=DEV)
    K = torch.tensor([[20.0, 20.0, 8.0, 8.0]], device=DEV).expand(B, 4).contiguous()
    kw = dict(lights=LIGHTS, ambient=0.1, smooth=True)
    big = render_meshes(v, f, K, (16, 16), **kw)
    for n in (B - 1, 0):
        one = render_meshes(v[n:n + 1], f, K[:1], (16, 16), **kw)
        for k in big:
            want = torch.where(one[k][0] >= 0, one[k][0] + n, one[k][0]) if k == "mesh_id" else one[k][0]     # (mesh index in the call)
            assert torch.equal(big[k][n], want), (n, k)
    assert (big["face_id"][B - 1] >= 0).sum() > 20
    del v, big
    torch.cuda.empty_cache()


# ---- 7. the host API -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("view", ["front", "left", "right", "back", "half_left", "half_right_above", "bottom", "above", "half_back_bottom"])
def test_render_mesh_over_the_demo_canvas(view):
    from dposer_amd.body_model import visual
    X, F = render_ref.body_torus()
    img = np.random.RandomState(2).randint(0, 256, (512, 384, 3)).astype(np.float64)
    out = visual.render_mesh(img, X, F, {"focal": list(FOCAL), "princpt": list(PRINCPT)}, view=view)
    assert out.dtype == np.float32 and out.shape == (512, 384, 3)
    T = visual.render_mesh_transform(X.astype(np.float64).mean(0), *visual.parse_view(view))
    ref = render_ref.render(X[None], F, [*FOCAL, *PRINCPT], 512, 384, transforms=T[None].astype(np.float32),
                            base_color=visual.RENDER_MESH_COLOR, lights=[(0, 0, 0, -1, *[visual.RENDER_MESH_LIGHT] * 3)] * 3,
                            ambient=visual.RENDER_MESH_AMBIENT)
    cov, ok = ref["covered"][0], ~ref["ambiguous"][0]
    unc = ~cov & ok
    assert np.array_equal(out[unc], img[unc].astype(np.float32))
    d = np.abs(out[cov & ok] - ref["rgb255"][0][cov & ok])
    assert d.max() <= 1.5 and (cov & ok).sum() > 20000


def _stats():
    return {"mean_poses": torch.zeros(63), "std_poses": torch.full((63,), 0.4), "min_poses": -torch.ones(63), "max_poses": torch.ones(63)}


@pytest.mark.parametrize("faster", [False, True])
@pytest.mark.parametrize("convert", [True, False])
def test_multiple_render_as_demo_calls_it(tmp_path, faster, convert):
    from functools import partial
    import dposer_amd
    dposer_amd.install_reference_aliases()
    from lib.body_model.visual import multiple_render
    from dposer_amd.body_model.body_model import BodyModel
    from dposer_amd.body_model.synthetic import make_synthetic_smplx_asset
    from dposer_amd.dataset.AMASS import Posenormalizer
    bm = BodyModel(make_synthetic_smplx_asset(seed=0)).to(DEV)
    nz = Posenormalizer(_stats(), device=DEV, normalize=True, min_max=False, rot_rep="axis")
    bg_img = np.ones([512, 384, 3]) * 255
    save_renders = partial(multiple_render, bg_img=bg_img, focal=[1500, 1500], princpt=[200, 192], device=DEV)   # demo.py:74
    samples = torch.as_tensor(np.random.RandomState(0).standard_normal((3, 63)).astype(np.float32) * 0.5, device=DEV)
    save_renders(samples, nz, bm, str(tmp_path), "generated_sample{}.png", convert=convert, faster=faster)
    save_renders(samples, nz, bm, str(tmp_path / "m"), "sample{}_masked.png", convert=convert, faster=faster, idx_map=[4, 0, 2])
    assert sorted(os.listdir(tmp_path / "m")) == ["sample1_masked.png", "sample3_masked.png", "sample5_masked.png"]
    names = sorted(n for n in os.listdir(tmp_path) if n.endswith(".png"))
    assert names == [f"generated_sample{k}.png" for k in (1, 2, 3)]
    imgs = [render_ref.decode_png((tmp_path / n).read_bytes()) for n in names]
    want = (256, 256, 3) if faster else (512, 384, 3)
    for a in imgs:
        assert a.shape == want
        assert (a != 255).any(-1).mean() > 0.01                       # a body on the white canvas
    assert not np.array_equal(imgs[0], imgs[1])
    m = render_ref.decode_png((tmp_path / "m" / "sample5_masked.png").read_bytes())
    assert np.array_equal(m, imgs[0])


def test_renderer_front_view_with_three_people_and_a_background():
    from dposer_amd.body_model import visual
    X, F = render_ref.body_torus()
    V = np.stack([X * 0.5 + [dx, 0, 5 + dz] for dx, dz in ((-0.9, 0.0), (0.0, 0.5), (0.9, 0.2))]).astype(np.float32)
    r = visual.Renderer(focal_length=500, img_w=320, img_h=240, faces=F)
    bg = np.random.RandomState(0).randint(0, 256, (240, 320, 3)).astype(np.uint8)
    out = r.render_front_view(V, bg_img_rgb=bg.copy())
    ref = render_ref.render(V, F, [500, 500, 160, 120], 240, 320, image_of_mesh=np.zeros(3, np.int64), base_color=(1, 1, 1),
                            lights=visual.renderer_lights(), smooth=True)
    cov, ok = ref["covered"][0], ~ref["ambiguous"][0]
    assert np.array_equal(out[~cov & ok], bg[~cov & ok])
    ids = ref["mesh_id"][0]
    for k in range(3):
        assert ((ids == k) & ok).sum() > 200
    plain = r.render_front_view(V)
    assert plain.dtype == np.uint8 and (plain[~cov & ok] == 0).all()
    assert len({tuple(plain[(ids == k) & ok].mean(0).round()) for k in range(3)}) == 3
    side = r.render_side_view(V)
    assert side.shape == (240, 320, 3) and (side != 0).any()
    r.delete()


def test_bad_inputs_are_refused():
    from dposer_amd._C import DPoserHipError
    from dposer_amd.body_model.visual import render_meshes
    v = torch.rand(2, 4, 3, device=DEV) + torch.tensor([0, 0, 2.0], device=DEV)
    f = torch.tensor([[0, 1, 2], [1, 2, 3]], device=DEV)
    K = torch.tensor([[10.0, 10, 4, 4]] * 2, device=DEV)
    with pytest.raises(DPoserHipError):
        render_meshes(v.cpu(), f.cpu(), K.cpu(), (8, 8))
    with pytest.raises(ValueError):
        render_meshes(v, torch.tensor([[0, 1, 4]], device=DEV), K, (8, 8))         # face index out of range
    with pytest.raises(ValueError):
        render_meshes(v, torch.tensor([[0, -1, 2]], device=DEV), K, (8, 8))
    with pytest.raises(ValueError):
        render_meshes(v[0], f, K, (8, 8))                                          # not [B, V, 3]
    with pytest.raises(ValueError):
        render_meshes(v, f[:, :2], K, (8, 8))
    with pytest.raises(ValueError):
        render_meshes(v, f, K[:, :3], (8, 8))
    with pytest.raises(ValueError):
        render_meshes(v, f, K, (0, 8))
    with pytest.raises(ValueError):
        render_meshes(v[:0], f, K, (8, 8))                                         # empty batch
    with pytest.raises(ValueError):
        render_meshes(v, f, K, (8, 8), image_of_mesh=torch.tensor([0, 5], device=DEV))
    got = render_meshes(v, f, K, (8, 8))
    assert got["rgb"].shape == (2, 8, 8, 3) and got["face_id"].dtype == torch.int32
