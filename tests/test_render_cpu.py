"""The mesh renderer without a GPU: the fill rule of the fp64 oracle (tests/render_ref.py), the camera matrices of the reference's presets
(render_mesh's views, faster_render, Renderer), the PNG writer, the C struct layout of dposer_render_args, the exported symbols, the
reference alias and the refusal of CPU tensors."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import render_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _coverage_count(P, H, W):
    """how many of the triangles P [n, 3, 3] (screen u, v, z) cover each pixel centre, by the oracle's rule."""
    A, D, own, _ = render_ref._edges(P)
    gj, gi = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    px = np.broadcast_to(gj.reshape(-1), (len(P), H * W))
    py = np.broadcast_to(gi.reshape(-1), (len(P), H * W))
    st, _, _, _ = render_ref._eval(P, A, D, own, px, py, 1e-9)
    return st.sum(0).reshape(H, W)


@pytest.mark.parametrize("flip", [False, True])
def test_square_split_on_a_diagonal_through_centres_covers_each_centre_once(flip):
    # corners on pixel centres: the diagonal and all four sides pass through centres
    c = np.array([[1.5, 1.5, 2.0], [7.5, 1.5, 2.0], [7.5, 7.5, 2.0], [1.5, 7.5, 2.0]])
    tris = np.array([[0, 1, 2], [0, 2, 3]]) if not flip else np.array([[2, 1, 0], [0, 3, 2]])
    n = _coverage_count(c[tris], 10, 10)
    assert n.max() == 1
    # top-left: the top row and the left column of centres are in, the bottom row and the right column out
    want = np.zeros((10, 10), int)
    want[1:7, 1:7] = 1
    assert np.array_equal(n, want)


def test_fan_around_a_centre_covers_it_once():
    ring = [(4.5 + 3 * np.cos(a), 4.5 + 3 * np.sin(a)) for a in np.linspace(0, 2 * np.pi, 7)[:-1]]
    pts = np.array([(4.5, 4.5)] + ring)
    P = np.array([[pts[0], pts[1 + k], pts[1 + (k + 1) % 6]] for k in range(6)])
    P = np.concatenate([P, np.full((6, 3, 1), 3.0)], -1)
    n = _coverage_count(P, 10, 10)
    assert n[4, 4] == 1 and n.max() == 1


def _trimesh_sequence(centroid, view):
    """visual.py:134-181 with 4x4 homogeneous matrices (trimesh.transformations' conventions), then the GL -> OpenCV flip."""
    def tr(t):
        m = np.eye(4)
        m[:3, 3] = t
        return m

    def rot(angle, axis):
        axis = np.asarray(axis, float) / np.linalg.norm(axis)
        K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        m = np.eye(4)
        m[:3, :3] = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K
        return m
    side = 45 if "half" in view else 90
    a = -side if "left" in view else side if "right" in view else 180 if "back" in view else 0
    p = 30 if "above" in view else -30 if "bottom" in view else 0
    M = tr(centroid) @ rot(np.radians(p), [1, 0, 0]) @ rot(np.radians(a), [0, 1, 0]) @ tr(-np.asarray(centroid))
    M = tr([0, 0, -7]) @ M
    return (np.diag([1.0, -1.0, -1.0, 1.0]) @ M)[:3]


VIEWS = ["front", "left", "right", "back", "half_left", "half_right", "half_front_above", "left_bottom", "half_back_above", "right_above",
         "bottom", "above"]


@pytest.mark.parametrize("view", VIEWS)
def test_render_mesh_view_matrices_match_the_reference_sequence(view):
    from dposer_amd.body_model import visual
    c = np.array([0.1, -0.3, 0.05])
    T = visual.render_mesh_transform(c, *visual.parse_view(view))
    assert np.allclose(T, _trimesh_sequence(c, view), atol=1e-12)


def test_random_view_uses_pythons_random_like_the_reference():
    import random
    from dposer_amd.body_model import visual
    random.seed(5)
    got = [visual.parse_view("random") for _ in range(20)]
    random.seed(5)
    want = []
    for _ in range(20):
        s, d, h = random.choice(["half", ""]), random.choice(["left", "right", "front", "back"]), random.choice(["above", "bottom", ""])
        want.append(visual.parse_view("_".join(o for o in (s, d, h) if o)))
    assert got == want and len(set(got)) > 3


def test_faster_camera_is_pytorch3d_look_at_2_0_0_with_60_degree_fov():
    from dposer_amd.body_model import visual
    T, K = visual.faster_camera()
    proj = lambda X: (lambda c: (K[0] * c[0] / c[2] + K[2], K[1] * c[1] / c[2] + K[3], c[2]))(T[:, :3] @ X + T[:, 3])
    assert np.allclose(proj(np.zeros(3)), (128, 128, 2))
    u, v, _ = proj(np.array([0.1, 0.0, 0.0]))
    assert u > 128                                       # world +x to the right of the image
    u, v, _ = proj(np.array([0.0, 0.1, 0.0]))
    assert v < 128                                       # world +y up
    # the top edge of the 60-degree frustum at the origin's depth
    u, v, _ = proj(np.array([0.0, 2 * np.tan(np.radians(30)), 0.0]))
    assert abs(v) < 1e-9


def test_renderer_lights_and_identity_camera():
    from dposer_amd.body_model import visual
    L = np.array(visual.renderer_lights(), float)
    assert np.allclose(L[:, 0], 0)
    s = np.sqrt(0.5)
    assert np.allclose(L[0, 1:4], [0, -s, -s]) and np.allclose(L[1, 1:4], [s, 0, -s])
    # the reference's mesh flip about x (rotation 180) followed by the GL camera (y, z negated) is the identity
    flip = visual.rotation_x(180)
    assert np.allclose(np.diag([1, -1, -1]) @ flip, np.eye(3))


def test_png_round_trip(tmp_path):
    from dposer_amd.body_model import visual
    a = np.random.RandomState(0).randint(0, 256, (37, 53, 3)).astype(np.uint8)
    p = tmp_path / "x.png"
    visual.write_image(str(p), a)
    assert np.array_equal(render_ref.decode_png(p.read_bytes()), a)
    with pytest.raises(ValueError):
        visual.encode_png(a.astype(np.float32))


def test_save_obj_writes_the_reference_format(tmp_path):
    from dposer_amd.body_model import visual
    v = np.array([[0.5, 1.0, -2.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], np.float32)
    f = np.array([[0, 1, 2]])
    p = tmp_path / "m.obj"
    visual.save_obj(v, f, str(p))
    assert p.read_text().splitlines() == ["v 0.5 1.0 -2.0", "v 1.0 0.0 0.0", "v 0.0 1.0 0.0", "f 1/1 2/2 3/3"]


def test_render_args_struct_matches_the_header_layout(tmp_path):
    """dposer_render_args as gcc lays it out against its ctypes mirror (the probe of test_mesh_si_cpu.py)."""
    import ctypes as C
    from dposer_amd import _C
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    cname, ct = "dposer_render_args", _C.RenderArgs
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dposer_hip.h"', 'int main(void) {',
             f'  printf("size %zu\\n", sizeof({cname}));']
    lines += [f'  printf("{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in ct._fields_]
    lines += ['  return 0;', '}']
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict((a, int(b)) for a, b in (ln.split() for ln in subprocess.check_output([str(exe)], text=True).splitlines()))
    assert got["size"] == C.sizeof(ct)
    for f, _ in ct._fields_:
        assert got[f] == getattr(ct, f).offset, f


def test_render_symbols_are_exported_and_scratch_is_bounded():
    from dposer_amd import _C
    names = ("dposer_render_meshes", "dposer_render_scratch_bytes")
    out = subprocess.check_output(["nm", "-D", "--defined-only", _C.LIB_PATH], text=True)
    syms = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for n in names:
        assert n in _C.SIGNATURES and n in syms, n
    l = _C.lib()
    B, V, F = 500, 10475, 20908
    s = l.dposer_render_scratch_bytes(B, V, F, B, 384, 512)
    assert s >= 5 * B * F * 4 + 3 * B * V * 16
    assert s < 5 * B * F * 4 + 3 * B * V * 16 + B * F * 16 + 4 * B * 13 * 16 * 4 + 8192
    assert l.dposer_render_scratch_bytes(1, 3, 1, 1, 0, 5) == 0


def test_reference_alias_resolves():
    import dposer_amd
    dposer_amd.install_reference_aliases()
    from lib.body_model.visual import Renderer, faster_render, multiple_render, render_mesh, save_obj  # noqa: F401
    from dposer_amd.body_model import visual
    assert render_mesh is visual.render_mesh and Renderer is visual.Renderer


def test_cpu_tensors_are_refused():
    from dposer_amd._C import DPoserHipError
    from dposer_amd.body_model.visual import render_meshes
    v = torch.zeros(1, 3, 3)
    with pytest.raises(DPoserHipError):
        render_meshes(v, torch.tensor([[0, 1, 2]]), [1, 1, 0, 0], (4, 4))
