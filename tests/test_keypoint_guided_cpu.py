"""The rule of the keypoint-residual stage and of DPS on observed 2D keypoints (tests/keypoint_guided_ref.py) on the CPU -- against the
reference's own reprojection loss (golden g34) and against central differences -- the host checks of the three Python functions, and what
dposer_keypoint_guide_stage / dposer_keypoint_guided_sampler export and refuse without a GPU: every refusal is an argument check (nothing
is launched) and its message starts with the name of the entry that was called."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import joint_guided_ref as jg
import keypoint_guided_ref as kg
import rot_ref as rr
from dposer_amd import _C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG, UNSUPPORTED = -1, -2
FAKE = C.c_void_p(0x1000)
MISALIGNED = C.c_void_p(0x1010)
TIMES = (C.c_float * 66)(*[1.0 - i / 80.0 for i in range(66)])
torch.set_num_threads(8)


def _jrest():
    a = rr.body_asset()
    return torch.tensor(a["J_regressor"].astype(np.float64) @ a["v_template"].astype(np.float64))


def test_the_rules_per_entry_terms_are_the_references_reprojection_loss():
    """g34: body_fitting_loss(..., output='reprojection') of the reference, computed there in float32 -- 1e-5 relative is its rounding."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "g34_reprojection.npz"))
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))
    conf, center = t(g["joints_conf"]), t(g["camera_center"])
    assert g["model_joints"].shape == (2, 4, 22, 3) and float(g["model_joints"][..., 2].min()) >= 2.0 and bool((conf == 0).any())
    assert [float(f) for f in g["focal"]] == [5000.0, 1000.0]
    for k, f in enumerate(g["focal"]):
        want = g["reprojection"][k].astype(np.float64)
        joints, kp = t(g["model_joints"][k]), t(g["keypoints"][k])
        got = (conf ** 2 * kg.reprojection_terms(joints, kp, torch.full((4,), float(f), dtype=torch.float64), center, float(g["sigma"]))).numpy()
        assert want.shape == (4, 22) and want.max() > 1e3                                  # outliers: gmof bends (sigma^2 = 1e4 per axis)
        assert (np.abs(got - want) <= 1e-5 * np.abs(want)).all(), float((np.abs(got - want) / np.maximum(np.abs(want), 1e-30)).max())
        assert not got[conf.numpy() == 0].any()


def _stage_kw(B, n_obs=22, rows=None, seed=0, conf=True, focal=5000.0, sigma=100.0, z=4.0, z_near=0.1):
    """A keypoint observation in float64: the projection of a random body + 10 px noise, camera 3..5 m away (``z``: the mean)."""
    rs = np.random.RandomState(seed)
    a, b = torch.tensor(rs.standard_normal(63) * 0.1), torch.tensor(rs.uniform(0.2, 0.5, 63))
    root = torch.tensor(rs.standard_normal((B, 3)) * 0.3)
    cam = torch.tensor(np.concatenate([rs.standard_normal((B, 2)) * 0.2, rs.uniform(z - 1, z + 1, (B, 1))], axis=1))
    J = jg.fk22(jg.denormalise(torch.tensor(rs.standard_normal((B, 63)) * 0.5), 1, a, b), root, _jrest(), cam)
    idx = list(range(n_obs)) if rows is None else rows
    center = torch.tensor([[500.0, 400.0]]).double().repeat(B, 1)
    fo = torch.full((B,), focal, dtype=torch.float64)
    kp = fo[:, None, None] * J[:, idx, :2] / J[:, idx, 2:3] + center[:, None] + torch.tensor(rs.standard_normal((B, n_obs, 2)) * 10.0)
    c = torch.tensor(rs.uniform(0.2, 1.5, (B, n_obs))) if conf else None
    return dict(mode=1, a=a, b=b, root=root, transl=cam, j_rest=_jrest(), kp=kp, conf=c, rows=rows, focal=fo, center=center, sigma=sigma, z_near=z_near)


@pytest.mark.parametrize("sigma", [100.0, 0.0])
def test_v_is_half_the_gradient_of_s_by_central_differences(sigma):
    B = 3
    kw = _stage_kw(B, n_obs=3, rows=[20, 15, 21], seed=1, sigma=sigma)
    y0 = torch.tensor(np.random.RandomState(2).standard_normal((B, 63)))
    s, v, live = kg.keypoint_stage(y0, **kw)
    assert bool(live.all()) and float(s.min()) > 0
    h = 1e-6
    for col in (0, 7, 31, 47, 62):
        e = torch.zeros(63, dtype=torch.float64)
        e[col] = h
        fd = (kg.stage_sum(y0 + e, **kw) - kg.stage_sum(y0 - e, **kw)) / (2 * h)
        assert float((0.5 * fd - v[:, col]).abs().max()) < 1e-7 * max(1.0, float(v.abs().max()))
    assert float(v.abs().max()) > 0


def test_dead_entries_holding_nan_and_joints_behind_the_plane_change_nothing():
    B = 4
    kw = _stage_kw(B, seed=3)
    y0 = torch.tensor(np.random.RandomState(4).standard_normal((B, 63)))
    dead = torch.tensor(np.random.RandomState(5).uniform(size=(B, 22)) < 0.4)
    dead[1] = True                                               # a row without a live entry
    conf0 = torch.where(dead, torch.zeros_like(kw["conf"]), kw["conf"])
    s0, v0, live0 = kg.keypoint_stage(y0, **dict(kw, conf=conf0))
    assert torch.equal(live0, ~dead)
    for bad_c in (0.0, -2.0, float("nan")):
        conf = torch.where(dead, torch.full_like(conf0, bad_c), conf0)
        kp = torch.where(dead[..., None], torch.full_like(kw["kp"], float("nan")), kw["kp"])
        s, v, _ = kg.keypoint_stage(y0, **dict(kw, conf=conf, kp=kp))
        assert bool(torch.isfinite(s).all()) and bool(torch.isfinite(v).all())
        assert torch.equal(s, s0) and torch.equal(v, v0)
    assert float(s0[1]) == 0.0 and not bool(v0[1].any())
    # a camera inside the body: the joints at or behind z_near drop out of s and v, exactly as if their confidence were 0
    near = dict(kw, transl=torch.tensor([[0.0, 0.0, 0.3]]).double().repeat(B, 1))
    terms, live, J = kg.stage_terms(y0, **near)
    behind = J[..., 2] <= near["z_near"]
    assert bool(behind.any()) and bool((~behind).any()) and torch.equal(live, ~behind)
    s1, v1, _ = kg.keypoint_stage(y0, **near)
    s2, v2, _ = kg.keypoint_stage(y0, **dict(near, conf=torch.where(behind, torch.zeros_like(kw["conf"]), kw["conf"])))
    assert bool(torch.isfinite(v1).all()) and torch.equal(s1, s2) and torch.equal(v1, v2)


def test_the_residual_order_keeps_the_observations_digits():
    """ru = focal (X / Z) - (k - centre): in float32 the rule loses no more than a few ulp of a pixel coordinate (~500 px -> 6e-5 px)."""
    kw = _stage_kw(5, seed=6)
    y0 = torch.tensor(np.random.RandomState(7).standard_normal((5, 63)))
    s64, _, _ = kg.keypoint_stage(y0, **kw)
    f = lambda v: v.float() if torch.is_tensor(v) and v.is_floating_point() else v
    s32, _, _ = kg.keypoint_stage(y0.float(), **{k: f(v) for k, v in kw.items()})
    assert float(((s32.double() - s64).abs() / s64).max()) < 1e-4


# ---- host checks of the Python surface -----------------------------------------------------------------------------------------------------------
def _py_problem(B=4, n=3):
    return dict(y0=torch.zeros(B, 63), kp=torch.zeros(B, n, 2), cam=torch.tensor([[0.0, 0.0, 4.0]]).repeat(B, 1), cen=torch.zeros(B, 2))


def test_host_checks_of_keypoint_residual_stage():
    from dposer_amd.tasks.completion import keypoint_residual_stage as stage
    q = _py_problem()
    ok = dict(cam_t=q["cam"], camera_center=q["cen"])
    with pytest.raises(ValueError, match=r"y0 must be \[B, 63\]"):
        stage(None, None, torch.zeros(4, 126), q["kp"], **ok)
    with pytest.raises(ValueError, match=r"keypoints2d must be \[4, 1\.\.22, 2\]"):
        stage(None, None, q["y0"], torch.zeros(4, 3, 3), **ok)
    with pytest.raises(ValueError, match=r"keypoints2d must be"):
        stage(None, None, q["y0"], torch.zeros(4, 23, 2), **ok)
    with pytest.raises(ValueError, match=r"cam_t must be \[4, 3\]"):
        stage(None, None, q["y0"], q["kp"], cam_t=q["cam"][:2], camera_center=q["cen"])
    with pytest.raises(ValueError, match=r"camera_center must be \[4, 2\]"):
        stage(None, None, q["y0"], q["kp"], cam_t=q["cam"], camera_center=torch.zeros(4, 3))
    with pytest.raises(ValueError, match="z_near"):
        stage(None, None, q["y0"], q["kp"], z_near=0.0, **ok)
    with pytest.raises(ValueError, match="focal_length"):
        stage(None, None, q["y0"], q["kp"], focal_length=torch.ones(3), **ok)
    with pytest.raises(ValueError, match="sigma must be"):
        stage(None, None, q["y0"], q["kp"], sigma=1e-20, **ok)
    with pytest.raises(ValueError, match="keypoints2d observes 3"):
        stage(None, None, q["y0"], q["kp"], obs_joints=[1, 2], **ok)
    with pytest.raises(ValueError, match="distinct"):
        stage(None, None, q["y0"], q["kp"], obs_joints=[4, 4, 5], **ok)
    with pytest.raises(ValueError, match=r"\[0, 22\)"):
        stage(None, None, q["y0"], q["kp"], obs_joints=[4, 22, 5], **ok)
    with pytest.raises(ValueError, match=r"keypoints_conf must be \[4, 3\]"):
        stage(None, None, q["y0"], q["kp"], keypoints_conf=torch.ones(4, 2), **ok)
    with pytest.raises(_C.DPoserHipError):                      # CPU tensors raise, as everywhere -- after the host checks
        stage(None, None, q["y0"], q["kp"], **ok)


def test_host_checks_of_the_sampler_and_of_sample_from_keypoints():
    from dposer_amd.algorithms.advanced import sampling, sde_lib
    from dposer_amd.tasks.completion import sample_from_keypoints
    sub = sde_lib.subVPSDE(0.1, 20.0, 10)
    with pytest.raises(ValueError, match="norm scope"):
        sampling.get_keypoint_guided_sampler(sub, (4, 63), None, None, norm="row")
    with pytest.raises(ValueError, match="63"):
        sampling.get_keypoint_guided_sampler(sub, (4, 126), None, None)
    with pytest.raises(ValueError, match="z_near"):
        sampling.get_keypoint_guided_sampler(sub, (4, 63), None, None, z_near=-1.0)
    q = _py_problem()
    fn = sampling.get_keypoint_guided_sampler(sub, (4, 63), None, None, device="cpu")
    with pytest.raises(ValueError, match=r"keypoints2d must be \[4, 1\.\.22, 2\]"):
        fn(None, torch.zeros(3, 3, 2), cam_t=q["cam"], camera_center=q["cen"])
    with pytest.raises(ValueError, match="distinct"):
        fn(None, q["kp"], obs_joints=[1, 1, 2], cam_t=q["cam"], camera_center=q["cen"])
    with pytest.raises(ValueError, match="start_step"):
        fn(None, q["kp"], cam_t=q["cam"], camera_center=q["cen"], start_step=11)
    with pytest.raises(ValueError, match="noise"):
        fn(None, q["kp"], cam_t=q["cam"], camera_center=q["cen"], noise=torch.zeros(9, 1, 4, 63))
    with pytest.raises(TypeError):                               # the camera is not optional
        fn(None, q["kp"])
    with pytest.raises(_C.DPoserHipError):
        fn(None, q["kp"], cam_t=q["cam"], camera_center=q["cen"], z=torch.zeros(4, 63))
    kw = dict(cam_t=q["cam"], camera_center=q["cen"])
    with pytest.raises(ValueError, match=r"keypoints2d must be \[B, n_obs, 2\]"):
        sample_from_keypoints(None, sub, None, None, torch.zeros(4, 3, 3), **kw)
    with pytest.raises(ValueError, match="hypo"):
        sample_from_keypoints(None, sub, None, None, q["kp"], hypo=0, **kw)
    with pytest.raises(ValueError, match=r"gt_poses must be \[4, 63\]"):
        sample_from_keypoints(None, sub, None, None, q["kp"], gt_poses=torch.zeros(4, 66), **kw)
    with pytest.raises(ValueError, match=r"\[0, 22\)"):
        sample_from_keypoints(None, sub, None, None, q["kp"], obs_joints=[0, 1, 30], **kw)


# ---- exports and refusals ------------------------------------------------------------------------------------------------------------------------
NAMES = ("dposer_keypoint_guide_stage", "dposer_keypoint_guide_stage_scratch_bytes", "dposer_keypoint_guided_sampler",
         "dposer_keypoint_guided_scratch_bytes")


def test_the_entries_are_exported_declared_and_bound():
    lib = _C.lib()
    header = open(os.path.join(ROOT, "include", "dposer_hip.h")).read()
    for name in NAMES:
        assert hasattr(lib, name) and name in _C.SIGNATURES and f" {name}(" in header, name
    assert "fitting_losses.py:6-47" in header and ":69-75" in header
    assert lib.dposer_keypoint_guide_stage_scratch_bytes(7) == 7 * 522 * 4 and lib.dposer_keypoint_guide_stage_scratch_bytes(0) == 0
    assert lib.dposer_keypoint_guided_scratch_bytes(7) == 7 * (522 + 127) * 4 and lib.dposer_keypoint_guided_scratch_bytes(0) == 0


@pytest.fixture(scope="module")
def body():
    lib = _C.lib()
    h = C.c_void_p()
    assert lib.dposer_body_create(C.byref(_C.BodyDesc(55, 1000, 10, 0, 0)), (C.c_int32 * 55)(*jg.SMPLX_PARENTS), C.byref(h)) == 0
    yield h
    lib.dposer_body_destroy(h)


@pytest.fixture(scope="module")
def nets():
    lib = _C.lib()
    hs = {}
    for D in (63, 126):
        h = C.c_void_p()
        assert lib.dposer_scorefc_create(C.byref(_C.ScoreFCDesc(D, 1024, 512, 2, _C.EMB_POSITIONAL, 1, 1000, _C.PREC_FP32, 0.1)), C.byref(h)) == 0
        hs[D] = h
    yield hs
    for h in hs.values():
        lib.dposer_scorefc_destroy(h)


def _sde(kind=_C.SDE_SUBVP):
    return C.byref(_C.SdeDesc(kind, 1000, 0.1, 20.0, 1.0))


def _stage_args(o):
    g = lambda k, d=FAKE: o.get(k, d)
    return [o["body"], g("y0"), g("data_dim", 63), g("norm_mode", 1), FAKE, FAKE, None, None, g("j_rest"), 0, g("kp"), None, None, g("n_obs", 3),
            g("focal"), g("center"), g("sigma", 100.0), g("z_near", 0.1), g("s"), g("v"), g("scratch"), g("batch", 16), None]


def _sampler_args(o):
    g = lambda k, d=FAKE: o.get(k, d)
    return [o["h"], FAKE, FAKE, g("ws"), g("sde", _sde()), g("x"), FAKE, TIMES, 0, 3, o["body"], 1, FAKE, FAKE, None, None, g("j_rest"), 0, g("kp"), None,
            None, g("n_obs", 3), g("focal"), g("center"), g("sigma", 100.0), g("z_near", 0.1), g("norm_scope", 1), None, 0, None, g("traj_stride", 1), 1.0,
            g("flag"), g("scratch"), FAKE, FAKE, 16, None]


NAN = float("nan")
STAGE_CASES = [
    ("null handle", {"body": None}, BAD_ARG, "null handle"),
    ("null y0", {"y0": None}, BAD_ARG, "null argument"),
    ("null rest joints", {"j_rest": None}, BAD_ARG, "null argument"),
    ("null keypoints", {"kp": None}, BAD_ARG, "null argument"),
    ("null focal", {"focal": None}, BAD_ARG, "null argument"),
    ("null center", {"center": None}, BAD_ARG, "null argument"),
    ("null s", {"s": None}, BAD_ARG, "null argument"),
    ("null v", {"v": None}, BAD_ARG, "null argument"),
    ("a 126-wide pose", {"data_dim": 126}, UNSUPPORTED, "rot6d"),
    ("data_dim 64", {"data_dim": 64}, BAD_ARG, "data_dim must be 63"),
    ("norm_mode 3", {"norm_mode": 3}, BAD_ARG, "bad normaliser"),
    ("n_obs 0", {"n_obs": 0}, BAD_ARG, "n_obs must be in 1..22"),
    ("n_obs 23", {"n_obs": 23}, BAD_ARG, "n_obs must be in 1..22"),
    ("z_near 0", {"z_near": 0.0}, BAD_ARG, "z_near must be positive"),
    ("z_near negative", {"z_near": -0.1}, BAD_ARG, "z_near must be positive"),
    ("z_near nan", {"z_near": NAN}, BAD_ARG, "z_near must be positive"),
    ("sigma nan", {"sigma": NAN}, BAD_ARG, "sigma must be <= 0 (no robustifier) or in"),
    ("sigma whose square underflows", {"sigma": 1e-20}, BAD_ARG, "sigma must be <= 0 (no robustifier) or in"),
    ("sigma whose square overflows", {"sigma": 1e20}, BAD_ARG, "sigma must be <= 0 (no robustifier) or in"),
    ("empty batch", {"batch": 0}, BAD_ARG, "batch must be positive"),
    ("null scratch", {"scratch": None}, BAD_ARG, "scratch must be non-null and 16-byte aligned"),
    ("misaligned scratch", {"scratch": C.c_void_p(0x1008)}, BAD_ARG, "scratch must be non-null and 16-byte aligned"),
]
SAMPLER_CASES = [
    ("null handle", {"h": None}, BAD_ARG, "null argument"),
    ("misaligned workspace", {"ws": MISALIGNED}, BAD_ARG, "packed / workspace must be 256-byte aligned"),
    ("null sde", {"sde": None}, BAD_ARG, "null argument"),
    ("null state", {"x": None}, BAD_ARG, "null argument"),
    ("null body", {"body": None}, BAD_ARG, "body, j_rest, keypoints, focal and center are required"),
    ("null rest joints", {"j_rest": None}, BAD_ARG, "body, j_rest, keypoints, focal and center are required"),
    ("null keypoints", {"kp": None}, BAD_ARG, "body, j_rest, keypoints, focal and center are required"),
    ("null focal", {"focal": None}, BAD_ARG, "body, j_rest, keypoints, focal and center are required"),
    ("null center", {"center": None}, BAD_ARG, "body, j_rest, keypoints, focal and center are required"),
    ("null flag", {"flag": None}, BAD_ARG, "nonfinite_step is required"),
    ("VE", {"sde": _sde(_C.SDE_VE)}, UNSUPPORTED, "the keypoint-guided sampler takes the continuous sub-VP and VP"),
    ("VE discrete", {"sde": _sde(_C.SDE_VE_DISCRETE)}, UNSUPPORTED, "continuous sub-VP and VP"),
    ("VP discrete", {"sde": _sde(_C.SDE_VP_DISCRETE)}, UNSUPPORTED, "continuous sub-VP and VP"),
    ("sde kind 9", {"sde": _sde(9)}, BAD_ARG, "unknown SDE kind"),
    ("a 126-wide network", {"D": 126}, UNSUPPORTED, "rot6d (126) is not supported"),
    ("norm_scope 2", {"norm_scope": 2}, BAD_ARG, "norm_scope must be 0 (batch) or 1 (sample)"),
    ("norm_scope -1", {"norm_scope": -1}, BAD_ARG, "norm_scope must be 0 (batch) or 1 (sample)"),
    ("n_obs 0", {"n_obs": 0}, BAD_ARG, "n_obs must be in 1..22"),
    ("n_obs 23", {"n_obs": 23}, BAD_ARG, "n_obs must be in 1..22"),
    ("z_near 0", {"z_near": 0.0}, BAD_ARG, "z_near must be positive"),
    ("z_near negative", {"z_near": -1.0}, BAD_ARG, "z_near must be positive"),
    ("sigma whose square underflows", {"sigma": 1e-20}, BAD_ARG, "sigma must be <= 0 (no robustifier) or in"),
    ("traj_stride 0", {"traj_stride": 0}, BAD_ARG, "traj_stride must be >= 1"),
    ("null scratch", {"scratch": None}, BAD_ARG, "scratch must be non-null and 16-byte aligned"),
    ("misaligned scratch", {"scratch": C.c_void_p(0x1008)}, BAD_ARG, "scratch must be non-null and 16-byte aligned"),
]


@pytest.mark.parametrize("what,over,code,text", STAGE_CASES, ids=[c[0].replace(" ", "_") for c in STAGE_CASES])
def test_stage_refusal(body, what, over, code, text):
    lib = _C.lib()
    o = {"body": body}
    o.update(over)
    rc = lib.dposer_keypoint_guide_stage(*_stage_args(o))
    msg = lib.dposer_last_error().decode()
    assert rc == code, (rc, msg)
    assert text in msg and msg.startswith("dposer_keypoint_guide_stage: "), msg


@pytest.mark.parametrize("what,over,code,text", SAMPLER_CASES, ids=[c[0].replace(" ", "_") for c in SAMPLER_CASES])
def test_sampler_refusal(body, nets, what, over, code, text):
    lib = _C.lib()
    o = {"body": body, "h": nets[over.get("D", 63)]}
    o.update({k: v for k, v in over.items() if k != "D"})
    rc = lib.dposer_keypoint_guided_sampler(*_sampler_args(o))
    msg = lib.dposer_last_error().decode()
    assert rc == code, (rc, msg)
    assert text in msg and msg.startswith("dposer_keypoint_guided_sampler: "), msg
