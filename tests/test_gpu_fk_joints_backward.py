"""dposer_fk_joints_backward (the gradient of the joints-only FK through the kinematic chain alone) against float64 autograd of the
chain rule in tests/joint_guided_ref.py, through the C ABI and through ``BodyModel.fk_joints(grad="chain")``.

Bound: relative L2 2e-4 per gradient, the one tests/test_gpu_fk.py holds dposer_lbs_backward's pose gradients to
(test_body_model_backward_vs_torch_autograd); by angle band, the bounds of tests/rot_ref.py as tests/test_gpu_rotations.py applies them
to the FK gradient.  One lane owns one pose and blocks are 64 lanes, so B in {1, 3, 65, 130} stands on both sides of the block edge and
of the small-batch threshold of the forward kernels the call runs first."""
import ctypes as C

import numpy as np
import pytest
import torch

import joint_guided_ref as jg
import rot_ref as rr
from gpu_common import DEV, t2n
from helpers import _log_measured

pytestmark = pytest.mark.gpu

BOUND = 2e-4
GUARD = 64                          # sentinel floats behind every output
SENTINEL = -12345.5
_SMPL_PARENTS = jg.SMPLX_PARENTS[:22] + (20, 21)
_SMPLH_PARENTS = (-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 22, 23, 20, 25, 26, 20, 28, 29, 20, 31, 32,
                  20, 34, 35, 21, 37, 38, 21, 40, 41, 21, 43, 44, 21, 46, 47, 21, 49, 50)
TREES = {"smpl": (_SMPL_PARENTS, (1, 23)), "smplh": (_SMPLH_PARENTS, (1, 21, 15, 15)), "smplx": (jg.SMPLX_PARENTS, (1, 21, 1, 1, 1, 15, 15))}


@pytest.fixture(scope="module")
def bm():
    from dposer_amd.body_model.body_model import BodyModel
    return BodyModel(rr.body_asset(), num_betas=10, num_expressions=0, model_type="smplx").to(DEV)


@pytest.fixture(scope="module")
def handles():
    from dposer_amd import _C
    lib = _C.lib()
    out = {}
    for name, (parents, _) in TREES.items():
        h = C.c_void_p()
        desc = _C.BodyDesc(len(parents), 100, 10, 0, 0)
        _C.check(lib.dposer_body_create(C.byref(desc), (C.c_int32 * len(parents))(*parents), C.byref(h)), "dposer_body_create")
        out[name] = h
    yield out
    for h in out.values():
        lib.dposer_body_destroy(h)


def _rel(got, want):
    want = np.asarray(want, dtype=np.float64)
    return float(np.linalg.norm(np.asarray(got, dtype=np.float64) - want) / max(np.linalg.norm(want), 1e-30))


def _guarded(n):
    """A device buffer of n floats with GUARD sentinel floats behind it, all sentinel-filled: (whole buffer, view of the n floats)."""
    buf = torch.full((n + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    return buf, buf[:n]


def _abi_backward(h, tree, full, jrest, dj, n_out, root_given=True, want_jrest=True):
    """One dposer_fk_joints_backward call on numpy inputs (full [B, J, 3], jrest [J, 3] or [B, J, 3], dj [B, n_out, 3]); returns the
    full-pose gradient [B, J, 3] (zeros where a segment was not given), the rest-joint gradient [B, n_out, 3] or None, after checking
    the guard words behind every output and behind the workspace."""
    from dposer_amd import _C
    lib = _C.lib()
    parents, segs = TREES[tree]
    B, J = full.shape[0], len(parents)
    ins, outs, first = [], [], 0
    for i, n in enumerate(segs):
        if i == 0 and not root_given:
            ins.append(None); outs.append(None)
        else:
            ins.append(torch.tensor(full[:, first:first + n].reshape(B, n * 3).copy(), device=DEV))
            outs.append(_guarded(B * n * 3))
        first += n
    segp = (C.c_void_p * len(segs))(*[None if t is None else t.data_ptr() for t in ins])
    dsegp = (C.c_void_p * len(segs))(*[None if o is None else o[1].data_ptr() for o in outs])
    segj = (C.c_int32 * len(segs))(*segs)
    jr, djd = torch.tensor(jrest, device=DEV), torch.tensor(dj, device=DEV)
    djr = _guarded(B * n_out * 3) if want_jrest else None
    nbytes = lib.dposer_fk_joints_backward_workspace_bytes(h, n_out, B)
    assert nbytes == B * n_out * 60
    ws = torch.full((nbytes + 4 * GUARD,), 0xAB, dtype=torch.uint8, device=DEV)
    _C.check(lib.dposer_fk_joints_backward(h, segp, segj, len(segs), _C.ptr(jr), 1 if jrest.ndim == 3 else 0, _C.ptr(djd), n_out * 3, n_out,
                                           dsegp, None if djr is None else _C.ptr(djr[1]), _C.ptr(ws), B, _C.stream_ptr()),
             "dposer_fk_joints_backward")
    torch.cuda.synchronize()
    assert bool((ws[nbytes:] == 0xAB).all()), "workspace guard"
    g = np.zeros((B, J, 3), dtype=np.float32)
    first = 0
    for n, o in zip(segs, outs):
        if o is not None:
            assert bool((o[0][B * n * 3:] == SENTINEL).all()), "pose-gradient guard"
            g[:, first:first + n] = t2n(o[1]).reshape(B, n, 3)
        first += n
    gj = None
    if djr is not None:
        assert bool((djr[0][B * n_out * 3:] == SENTINEL).all()), "rest-joint-gradient guard"
        gj = t2n(djr[1]).reshape(B, n_out, 3)
    return g, gj


def _case(tree, B, n_out, batched, seed, scale=0.4):
    parents, _ = TREES[tree]
    J = len(parents)
    rs = np.random.RandomState(seed)
    full = (rs.standard_normal((B, J, 3)) * scale).astype(np.float32)
    jrest = rs.standard_normal((J, 3)).astype(np.float32) * 0.3
    if batched:
        jrest = (jrest[None] + rs.standard_normal((B, J, 3)) * 0.05).astype(np.float32)
    dj = rs.standard_normal((B, n_out, 3)).astype(np.float32)
    return full, jrest, dj


def _rule(tree, full, jrest, dj, n_out, root_given=True):
    """float64 autograd of the chain: (d full pose [B, J, 3], d rest joints [B, n_out, 3] per pose)."""
    parents, _ = TREES[tree]
    B, J = full.shape[0], len(parents)
    f = torch.tensor(full, dtype=torch.float64)
    if not root_given:
        f[:, 0] = 0.0
    f = f.reshape(B, J * 3).requires_grad_(True)
    jr = torch.tensor(np.broadcast_to(jrest, (B, J, 3)).copy(), dtype=torch.float64, requires_grad=True)
    val = (jg.fk_chain(f, jr, parents, n_out) * torch.tensor(dj, dtype=torch.float64)).sum()
    gf, gj = torch.autograd.grad(val, [f, jr], allow_unused=True)          # (n_out == 1: the root's position is its rest joint)
    gf = np.zeros((B, J, 3)) if gf is None else gf.reshape(B, J, 3).numpy().copy()
    if not root_given:
        gf[:, 0] = 0.0
    assert float(gj[:, n_out:].abs().max()) == 0.0 if n_out < J else True
    return gf, gj[:, :n_out].numpy()


@pytest.mark.parametrize("batched", [False, True], ids=["shared rest joints", "batched rest joints"])
@pytest.mark.parametrize("n_out", [1, 10, 22, 55])
@pytest.mark.parametrize("B", [1, 3, 65, 130])
def test_parity_with_float64_autograd_of_the_chain(handles, B, n_out, batched):
    for root_given in (True, False):
        full, jrest, dj = _case("smplx", B, n_out, batched, seed=1000 * B + n_out)
        g, gj = _abi_backward(handles["smplx"], "smplx", full, jrest, dj, n_out, root_given)
        g2, gj2 = _abi_backward(handles["smplx"], "smplx", full, jrest, dj, n_out, root_given)
        assert np.array_equal(g, g2) and np.array_equal(gj, gj2)                 # two runs, the same bits
        want, want_j = _rule("smplx", full, jrest, dj, n_out, root_given)
        assert not g[:, n_out:].any()                                            # joints that were not evaluated: exact zeros
        first = 0 if root_given else 1
        if not want.any():
            assert not g.any()
        else:
            e = _rel(g[:, first:n_out], want[:, first:n_out])
            _log_measured(f"fk_joints_backward B={B} n_out={n_out} root={root_given} batched={batched} | d pose rel L2", e)
            assert e < BOUND, e
        ej = _rel(gj, want_j)
        _log_measured(f"fk_joints_backward B={B} n_out={n_out} root={root_given} batched={batched} | d j_rest rel L2", ej)
        assert ej < BOUND, ej
        assert np.isfinite(g).all() and np.isfinite(gj).all()


@pytest.mark.parametrize("tree", ["smpl", "smplh"])
def test_smpl_and_smplh_handles(handles, tree):
    for B in (3, 130):
        full, jrest, dj = _case(tree, B, 22, False, seed=77 + B)
        g, gj = _abi_backward(handles[tree], tree, full, jrest, dj, 22)
        want, want_j = _rule(tree, full, jrest, dj, 22)
        assert _rel(g[:, :22], want[:, :22]) < BOUND and _rel(gj, want_j) < BOUND
        assert not g[:, 22:].any()


def test_unwanted_outputs_are_not_written(handles):
    """NULL gradient pointers (a segment's, the rest joints') change nothing in the outputs that are wanted."""
    full, jrest, dj = _case("smplx", 65, 22, True, seed=5)
    g, _ = _abi_backward(handles["smplx"], "smplx", full, jrest, dj, 22)
    g2, none = _abi_backward(handles["smplx"], "smplx", full, jrest, dj, 22, want_jrest=False)
    assert none is None and np.array_equal(g, g2)


def _python_case(B, seed, n=22):
    rs = np.random.RandomState(seed)
    a = lambda *s, k=1.0: (rs.standard_normal(s) * k).astype(np.float32)
    return dict(pose=a(B, 63, k=0.4), root=a(B, 3, k=0.4), trans=a(B, 3), betas=a(B, 10, k=0.5), w=a(B, n, 3))


@pytest.mark.parametrize("with_root_and_trans", [True, False])
@pytest.mark.parametrize("n", [10, 22])
def test_autograd_surface_against_the_oracle_and_the_lbs_route(bm, n, with_root_and_trans):
    """BodyModel.fk_joints(grad="chain"): pose, root orientation, translation and betas (rest joints through the shape-blend backward)
    against float64 autograd of oracle/fk_torch.py, and against grad="lbs" (zero vertex gradient) under the same bound."""
    from oracle import fk_torch
    B = 65
    c = _python_case(B, 11 + n, n)
    names = ["pose", "betas"] + (["root", "trans"] if with_root_and_trans else [])
    w = torch.tensor(c["w"], device=DEV)
    got = {}
    for route in ("chain", "lbs"):
        t = {k: torch.tensor(c[k], device=DEV, requires_grad=True) for k in names}
        j = bm.fk_joints(t["pose"], root_orient=t.get("root"), trans=t.get("trans"), n_joints=n, betas=t["betas"], grad=route)
        assert j.shape == (B, n, 3)
        gs = torch.autograd.grad((j * w).sum(), [t[k] for k in names])
        got[route] = {k: t2n(g) for k, g in zip(names, gs)}
        got[route]["joints"] = t2n(j)
    assert np.array_equal(got["chain"]["joints"], got["lbs"]["joints"][:, :n]) or np.abs(got["chain"]["joints"] - got["lbs"]["joints"]).max() < 1e-5
    r = {k: torch.tensor(c[k], dtype=torch.float64, requires_grad=True) for k in names}
    _, jr = fk_torch.smplx_forward(rr.body_asset(), r["pose"], betas=r["betas"], global_orient=r.get("root"), transl=r.get("trans"))
    want = torch.autograd.grad((jr[:, :n] * torch.tensor(c["w"], dtype=torch.float64)).sum(), [r[k] for k in names])
    for k, wk in zip(names, want):
        e, e_lbs = _rel(got["chain"][k], wk.numpy()), _rel(got["chain"][k], got["lbs"][k])
        _log_measured(f"fk_joints grad=chain n={n} | d {k} vs float64 rel L2", e)
        _log_measured(f"fk_joints grad=chain n={n} | d {k} vs grad=lbs rel L2", e_lbs)
        assert e < BOUND and e_lbs < BOUND, (k, e, e_lbs)


def test_all_55_joints_with_hands_and_face(bm):
    from oracle import fk_torch
    B = 3
    rs = np.random.RandomState(9)
    keys = dict(body_pose=63, global_orient=3, jaw_pose=3, leye_pose=3, reye_pose=3, left_hand_pose=45, right_hand_pose=45)
    vals = {k: (rs.standard_normal((B, n)) * 0.4).astype(np.float32) for k, n in keys.items()}
    w = rs.standard_normal((B, 55, 3)).astype(np.float32)
    t = {k: torch.tensor(v, device=DEV, requires_grad=True) for k, v in vals.items()}
    j = bm.bm(joints_only=True, n_joints=55, grad="chain", **t).joints
    got = torch.autograd.grad((j * torch.tensor(w, device=DEV)).sum(), list(t.values()))
    r = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in vals.items()}
    _, jr = fk_torch.smplx_forward(rr.body_asset(), **r)
    want = torch.autograd.grad((jr[:, :55] * torch.tensor(w, dtype=torch.float64)).sum(), list(r.values()))
    for k, a, b in zip(keys, got, want):
        assert _rel(t2n(a), b.numpy()) < BOUND, k


@pytest.mark.parametrize("pattern", rr.PATTERNS)
def test_chain_gradient_by_band(bm, pattern):
    """The loss of tests/test_gpu_rotations.py::test_joint_gradient_by_band (a fixed linear functional of the 22 body joints) through
    grad="chain", in every angle band of tests/rot_ref.py -- zero pose, 1e-4, pi - 1e-3 and beyond 2 pi among them -- under the same
    yardstick-and-floor bounds."""
    ref = rr.body_reference(pattern)
    wj, _ = rr.body_weights()
    wj_d = torch.tensor(wj[:, :22].copy(), device=DEV)
    bad = []
    for band in rr.BAND_NAMES:
        root, body = rr.body_poses(pattern, band)
        r = torch.tensor(root, device=DEV, requires_grad=True)
        p = torch.tensor(body, device=DEV, requires_grad=True)
        val = (bm.fk_joints(p, root_orient=r, n_joints=22, grad="chain") * wj_d).sum()
        gr, gp = torch.autograd.grad(val, [r, p])
        g = np.concatenate([t2n(gr), t2n(gp)], axis=1)
        s = rr.band_rows(band)
        T, Y = ref["grad_joints_truth"][s], ref["grad_joints_yard"][s]
        lim = rr.bound(rr.max_abs(Y, T), rr.FLOOR_MAT * float(np.abs(T).max()))
        err = rr.max_abs(g, T)
        _log_measured(f"band {band} | {pattern} | d joints loss / d (root_orient, pose_body) via the chain | err / limit", float(err) / lim)
        if not err <= lim:
            bad.append((band, float(err), lim))
    assert not bad, bad


def test_zero_pose(bm):
    """All-zero pose and root: smplx's + 1e-8 keeps the rotation's gradient finite; parity with the float64 rule."""
    B = 3
    w = np.random.RandomState(2).standard_normal((B, 22, 3)).astype(np.float32)
    p = torch.zeros(B, 63, device=DEV, requires_grad=True)
    r = torch.zeros(B, 3, device=DEV, requires_grad=True)
    gr, gp = torch.autograd.grad((bm.fk_joints(p, root_orient=r, grad="chain") * torch.tensor(w, device=DEV)).sum(), [r, p])
    asset = rr.body_asset()
    jrest = torch.tensor(asset["J_regressor"].astype(np.float64) @ asset["v_template"].astype(np.float64))
    p6 = torch.zeros(B, 63, dtype=torch.float64, requires_grad=True)
    r6 = torch.zeros(B, 3, dtype=torch.float64, requires_grad=True)
    wr, wp = torch.autograd.grad((jg.fk22(p6, r6, jrest) * torch.tensor(w, dtype=torch.float64)).sum(), [r6, p6])
    assert _rel(t2n(gp), wp.numpy()) < BOUND and _rel(t2n(gr), wr.numpy()) < BOUND


def test_memory_of_a_forward_and_backward_at_4096_poses(bm):
    """No vertex-sized array anywhere: peak allocation across forward + backward grows by less than 16 KB per pose beyond the inputs
    and outputs (the LBS route keeps > 100 KB per pose)."""
    B = 4096
    c = _python_case(B, 3)
    p = torch.tensor(c["pose"], device=DEV, requires_grad=True)
    r = torch.tensor(c["root"], device=DEV, requires_grad=True)
    w = torch.tensor(c["w"], device=DEV)
    bm.fk_joints(p[:8], root_orient=r[:8], grad="chain").sum().backward()           # handle and caches exist
    p.grad = r.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    j = bm.fk_joints(p, root_orient=r, grad="chain")
    (j * w).sum().backward()
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - base
    io = 4 * B * (22 * 3 * 3 + 2 * 66)       # joints, their product with w and its gradient; the two pose gradients (twice: empty_like + .grad)
    _log_measured("fk_joints grad=chain forward + backward at 4096 poses | peak bytes per pose beyond the inputs", grown / B)
    assert grown < 16 * 1024 * B + io, grown / B
    assert p.grad is not None and bool(torch.isfinite(p.grad).all())


def test_the_default_route_is_still_the_lbs_function(bm):
    """grad="lbs" (the default) runs what it ran before: the same bits from the same call twice, with and without the keyword, and
    from _LBSFunction applied directly."""
    from dposer_amd.body_model.body_model import _LBSFunction
    B = 65
    c = _python_case(B, 21)
    w = torch.tensor(c["w"], device=DEV)

    def run(fn):
        p = torch.tensor(c["pose"], device=DEV, requires_grad=True)
        r = torch.tensor(c["root"], device=DEV, requires_grad=True)
        j = fn(p, r)
        return (j.detach().clone(),) + torch.autograd.grad((j * w).sum(), [r, p])

    core = bm.bm
    v_shaped, j_rest, batched = core.rest_shape(None, None)

    def direct(p, r):
        segs = dict(global_orient=r, body_pose=p)
        _, joints = _LBSFunction.apply(core, batched, v_shaped, j_rest, None, *[segs.get(name) for name, _ in core.segments])
        return joints[:, :22]

    a = run(lambda p, r: bm.fk_joints(p, root_orient=r))
    b = run(lambda p, r: bm.fk_joints(p, root_orient=r, grad="lbs"))
    d = run(direct)
    for x, y, z in zip(a, b, d):
        assert torch.equal(x, y) and torch.equal(x, z)
