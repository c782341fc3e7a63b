"""dposer_fk_joints_backward without a GPU: the entry and its byte query are exported, declared and bound; every malformed call is
refused by an argument check (nothing is launched: a launch attempt on a machine without a GPU would come back as DPOSER_ERR_HIP) with
a message that starts with the entry's name; and the float64 rule the GPU tests hold it to (tests/joint_guided_ref.py) is the
oracle's chain."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import joint_guided_ref as jg
from dposer_amd import _C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG = -1
FAKE = C.c_void_p(0x1000)
ENTRY = "dposer_fk_joints_backward"
QUERY = "dposer_fk_joints_backward_workspace_bytes"


@pytest.fixture(scope="module")
def body():
    lib = _C.lib()
    h = C.c_void_p()
    desc = _C.BodyDesc(55, 1000, 10, 0, 0)
    assert lib.dposer_body_create(C.byref(desc), (C.c_int32 * 55)(*jg.SMPLX_PARENTS), C.byref(h)) == 0
    yield h
    lib.dposer_body_destroy(h)


def test_the_entry_is_exported_declared_and_bound():
    lib = _C.lib()
    header = open(os.path.join(ROOT, "include", "dposer_hip.h")).read()
    for name in (ENTRY, QUERY):
        assert hasattr(lib, name), name
        assert name in _C.SIGNATURES, name
        assert f" {name}(" in header, name
    assert len(_C.SIGNATURES[ENTRY][1]) == 14 and _C.SIGNATURES[QUERY][0] is C.c_int64


def test_workspace_is_sixty_bytes_per_joint_and_pose(body):
    lib = _C.lib()
    assert lib.dposer_fk_joints_backward_workspace_bytes(body, 22, 4096) == 4096 * 22 * 60
    assert lib.dposer_fk_joints_backward_workspace_bytes(body, 55, 1) == 55 * 60
    assert lib.dposer_fk_joints_backward_workspace_bytes(body, 55, 1) < 16 * 1024          # the issue's bound per pose
    for h, n, b in ((None, 22, 8), (body, 0, 8), (body, 56, 8), (body, 22, 0)):
        assert lib.dposer_fk_joints_backward_workspace_bytes(h, n, b) == 0


def _call(o):
    nseg = o.get("nseg", 2)
    segj = (C.c_int32 * 8)(*o.get("segj", (1, 54)), *([0] * 6))
    segp = (C.c_void_p * 8)(FAKE, FAKE)
    dsegp = (C.c_void_p * 8)(FAKE, FAKE)
    return [o.get("h"), o.get("segp", segp), segj, nseg, o.get("j_rest", FAKE), 0, o.get("d_joints", FAKE), o.get("ld", 66), o.get("n_out", 22),
            o.get("dsegp", dsegp), None, o.get("ws", FAKE), o.get("batch", 8), None]


CASES = [
    ("null handle", {"h": None}, "null handle"),
    ("null pose segments", {"segp": None}, "null argument"),
    ("null rest joints", {"j_rest": None}, "null argument"),
    ("null joint gradient", {"d_joints": None}, "null argument"),
    ("null gradient list", {"dsegp": None}, "null argument"),
    ("no segments", {"nseg": 0}, "1..8 pose segments"),
    ("nine segments", {"nseg": 9}, "1..8 pose segments"),
    ("empty batch", {"batch": 0}, "batch must be positive"),
    ("n_out 0", {"n_out": 0}, "n_out must be in 1..num_joints"),
    ("n_out 56", {"n_out": 56, "ld": 168}, "n_out must be in 1..num_joints"),
    ("short gradient rows", {"ld": 65}, "d_joints_ld must be at least 3 * n_out"),
    ("null workspace", {"ws": None}, "workspace must be non-null and 16-byte aligned"),
    ("misaligned workspace", {"ws": C.c_void_p(0x1008)}, "workspace must be non-null and 16-byte aligned"),
    ("segments of another tree", {"segj": (1, 23)}, "pose segments must cover all joints"),
    ("a segment without joints", {"segj": (0, 55)}, "a pose segment has at least one joint"),
]


@pytest.mark.parametrize("what,over,text", CASES, ids=[c[0].replace(" ", "_") for c in CASES])
def test_refusal(body, what, over, text):
    lib = _C.lib()
    o = {"h": body}
    o.update(over)
    rc = lib.dposer_fk_joints_backward(*_call(o))
    msg = lib.dposer_last_error().decode()
    assert rc == BAD_ARG, (rc, msg)
    assert text in msg, msg
    assert msg.startswith(ENTRY + ": "), msg


def test_the_rule_is_the_oracles_chain():
    """tests/joint_guided_ref.py forms no vertex; its joints and their pose gradient are those of oracle/fk_torch.py in float64."""
    import rot_ref as rr
    from oracle import fk_torch
    asset = rr.body_asset()
    assert tuple(int(p) for p in asset["parents"]) == jg.SMPLX_PARENTS
    rs = np.random.RandomState(3)
    B = 4
    pose = torch.tensor(rs.standard_normal((B, 63)) * 0.5, requires_grad=True)
    root = torch.tensor(rs.standard_normal((B, 3)) * 0.5, requires_grad=True)
    tr = torch.tensor(rs.standard_normal((B, 3)))
    w = torch.tensor(rs.standard_normal((B, 22, 3)))
    jrest = torch.tensor(asset["J_regressor"].astype(np.float64) @ asset["v_template"].astype(np.float64))
    mine = jg.fk22(pose, root, jrest, tr)
    _, ref = fk_torch.smplx_forward(asset, pose, global_orient=root, transl=tr)
    assert float((mine - ref[:, :22]).detach().abs().max()) < 1e-13
    g_mine = torch.autograd.grad((mine * w).sum(), [root, pose])
    g_ref = torch.autograd.grad((ref[:, :22] * w).sum(), [root, pose])
    for a, b in zip(g_mine, g_ref):
        assert float((a - b).abs().max()) < 1e-12
    assert mine.shape == (B, 22, 3) and jg.fk_chain(torch.zeros(2, 165, dtype=torch.float64), jrest, jg.SMPLX_PARENTS, 55).shape == (2, 55, 3)


def test_grad_route_is_validated_before_any_device_work():
    import rot_ref as rr
    from dposer_amd.body_model.body_model import BodyModel
    bm = BodyModel(rr.body_asset(), num_betas=10, num_expressions=0, model_type="smplx")
    p = torch.zeros(2, 63)
    with pytest.raises(ValueError, match="grad must be"):
        bm.fk_joints(p, grad="mesh")
    with pytest.raises(ValueError, match="joints_only"):
        bm.bm(body_pose=p, grad="chain")
    with pytest.raises(_C.DPoserHipError):                      # CPU tensors raise, as everywhere
        bm.fk_joints(p, grad="chain")
