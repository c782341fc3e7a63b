"""GPU tests of the keypoint-residual stage (dposer_keypoint_guide_stage) and of DPS on observed 2D keypoints in one call
(dposer_keypoint_guided_sampler / sampling.get_keypoint_guided_sampler / tasks.completion.sample_from_keypoints) against the float64 rule
of tests/keypoint_guided_ref.py.

The camera of every problem: cam_t z in [3, 5] m, focal 1000 or 5000, centre (500, 400).  The synthetic body's longest root-to-joint chain
is 1.51 m, so no joint of any pose comes nearer than 1.4 m and depth never decides liveness, except in the one case built for it (cam_t
z = 0.3 m); the sampler tests assert min Z > 1 m on the rule's side.

Tolerances.  A pixel residual is focal / Z (~ 1000 .. 2000 px per metre) times a joint position, so an fp32 rounding of the chain is a visible
fraction of a residual, and in the sampler y0 = (x + sigma^2 score) / alpha is hundreds of units at large t (tests/test_gpu_joint_guided.py has
that story).  Every accuracy bound therefore has the form
    max(floor, K * e32),   e32 = the error of the same float64 rule evaluated in float32 on the same inputs,
with floor = 2e-4 for the stage (tests/test_gpu_fk.py's pose-gradient bound, for v and for s alike: rel-L2 over the batch) and
STEP_TOLS[prec] for a sampler step, and K = twice the worst measured e_lib / e32, rounded up (profiles/keypoint_guided_parity.md has the
measured ratios).  The library does the rule's fp32 arithmetic in another order: a ratio above 8 is a bug, not a K, and every test here
asserts that cap.  For the stage the cap is on the ratio with e32 FLOORED at the float32 unit roundoff 2^-24: for a single pose e32 of s is the
rounding of one number and can be far below it by luck (worst raw ratio 9.53 at e32 = 3.6e-8, floored 5.82).

bf16x3 and the forward.  bf16x3 runs the same fp32 stage behind a network forward that is ~6 times less exact than fp32's (8e-6 against
1.4e-6 rel-L2), an error that e32 -- the rule in plain float32 -- does not contain.  Against the plain rule its worst e_lib / e32 is 28.72
(sub-VP, batch scope, index 50: e_lib 2.52e-4, e32 8.8e-6).  forced_errors isolates it: the float64 rule is stepped once more with the
LIBRARY's forward values at the same states substituted for its own (keypoint_guided_ref: score_shift; the Jacobian stays the rule's).
e_fwd, that step against the plain rule, is what the forward's error alone does: 2.92e-4 at that index -- the whole of e_lib -- and
e_lib / (e_fwd + e32) is at most 1.66 over all four runs.  So a bf16x3 step is held in two parts: the forward's rel-L2 at every listed state
<= STEP_TOLS["bf16x3"] (measured 6.7e-6 .. 1.06e-5), and the library's step against the rule ON THE LIBRARY'S FORWARD at
max(STEP_TOLS, K e32) with the cap of 8 (measured worst ratios 3.65, 5.73, 4.04, 2.67: K = 12); the two bound e_lib by the triangle inequality.
The guidance step of every sampler test is 0.7 * 4 / focal (``_gs``), not the 3D tests' 0.7: see there.
"""
import numpy as np
import pytest
import torch

import guided_ref as G
import joint_guided_ref as jg
import keypoint_guided_ref as kg
import rot_ref as rr
from gpu_common import DEV, make_model, t2n
from helpers import _log_measured, rel_err

pytestmark = pytest.mark.gpu
torch.set_num_threads(8)
TOLS = {"fp32": 1e-4, "bf16x3": 1e-4, "bf16": 1e-2}          # tests/test_gpu_guided_sampler.py: after a sampler run
STEP_TOLS = {"fp32": 1e-5, "bf16x3": 2e-5, "bf16": 2e-2}     # tests/test_gpu_guided_sampler.py: one guided step
STAGE_FLOOR = 2e-4                                           # tests/test_gpu_fk.py: pose gradients, rel-L2
# twice the worst measured ratio, rounded up (profiles/keypoint_guided_parity.md): stage 5.82 (floored e32); fp32 1.73; bf16x3 5.73 (on its forward)
K_STAGE = 12
K_E32 = {"fp32": 4, "bf16x3": 12}
GRAD_STEP = 0.7                                              # the 3D-joint tests' step, for a residual in metres


def _gs(focal):
    """The step for a residual in pixels: d px / d m = focal / Z, so GRAD_STEP times metres per pixel at the cameras' mean depth of 4 m moves the
    state about as far per index as the 3D-joint tests' step does (0.7 itself would throw every state hundreds of units out)."""
    return GRAD_STEP * 4.0 / float(focal)


U32 = 2.0 ** -24                                             # float32 unit roundoff: an e32 below it is luck, not accuracy
CENTER = (500.0, 400.0)
_MODELS = {}


def _dev(a, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def _model(seed, prec):
    if (seed, prec) not in _MODELS:
        _MODELS[(seed, prec)] = make_model(seed, precision=prec)
    return _MODELS[(seed, prec)]


def _sde(kind, N):
    from dposer_amd.algorithms.advanced import sde_lib
    return (sde_lib.subVPSDE if kind == "subvp" else sde_lib.VPSDE)(0.1, 20.0, N)


@pytest.fixture(scope="module")
def bm():
    from dposer_amd.body_model.body_model import BodyModel
    return BodyModel(rr.body_asset(), num_betas=10, num_expressions=0, model_type="smplx").to(DEV)


def _jrest():
    a = rr.body_asset()
    return a["J_regressor"].astype(np.float64) @ a["v_template"].astype(np.float64)


def _stats():
    rs = np.random.RandomState(4)
    return dict(mean_poses=torch.tensor(rs.standard_normal(63) * 0.1, dtype=torch.float32),
                std_poses=torch.tensor(rs.uniform(0.2, 0.5, 63), dtype=torch.float32),
                min_poses=torch.tensor(-rs.uniform(1.0, 2.0, 63), dtype=torch.float32),
                max_poses=torch.tensor(rs.uniform(1.0, 2.0, 63), dtype=torch.float32))


def _normalizer(kind):
    from dposer_amd.dataset.AMASS import Posenormalizer
    return Posenormalizer(_stats(), device=DEV, normalize=kind != "none", min_max=kind == "minmax", rot_rep="axis")


def _norm_tables(kind):
    """(mode, a, b) of the rule, float64."""
    st = {k: v.double() for k, v in _stats().items()}
    return {"none": (0, None, None), "zscore": (1, st["mean_poses"], st["std_poses"]), "minmax": (2, st["min_poses"], st["max_poses"])}[kind]


ROWS = {1: None, 3: [20, 15, 21], 22: None}


def _problem(B, n_obs, conf_kind, seed, *, norm_kind="zscore", focal=5000.0, sigma=100.0, cam_z=(3.0, 5.0), z_near=0.1):
    """A 2D-keypoint observation for B poses: the projection of a random body plus 10 px of noise; confidences None / random with zeros,
    negatives and NaN / that and row 0 all dead; NaN under every dead entry.  Everything the library reads is float32-exact."""
    rs = np.random.RandomState(seed)
    rows = ROWS[n_obs]
    idx = list(range(n_obs)) if rows is None else rows
    mode, a, b = _norm_tables(norm_kind)
    y_gt = torch.tensor(rs.standard_normal((B, 63)) * (0.5 if norm_kind != "none" else 0.2))
    root = (rs.standard_normal((B, 3)) * 0.3).astype(np.float32)
    cam = np.concatenate([rs.standard_normal((B, 2)) * 0.2, rs.uniform(cam_z[0], cam_z[1], (B, 1))], axis=1).astype(np.float32)
    J = jg.fk22(jg.denormalise(y_gt, mode, a, b), torch.tensor(root).double(), torch.tensor(_jrest()), torch.tensor(cam).double()).numpy()
    Z = np.where(np.abs(J[:, idx, 2:3]) > 1e-3, J[:, idx, 2:3], 1e-3)
    kp = (focal * J[:, idx, :2] / Z + np.array(CENTER) + rs.standard_normal((B, n_obs, 2)) * 10.0).astype(np.float32)
    conf = None
    if conf_kind != "none":
        conf = rs.uniform(0.2, 1.5, (B, n_obs)).astype(np.float32)
        dead = rs.uniform(size=(B, n_obs)) < 0.3
        conf[dead] = rs.choice(np.array([0.0, -1.0, np.nan], dtype=np.float32), size=int(dead.sum()))
        if conf_kind == "row dead":
            conf[0] = 0.0
        kp[~(conf > 0)] = np.nan
    return dict(kp=kp, conf=conf, rows=rows, root=root, cam=cam, center=np.tile(np.array(CENTER, dtype=np.float32), (B, 1)),
                focal=np.full(B, focal, dtype=np.float32), sigma=sigma, z_near=z_near, mode=mode, a=a, b=b, norm_kind=norm_kind)


def _rule_kw(q, dtype=torch.float64, tile=None):
    """The keyword arguments of the rule's stage behind y0, in ``dtype``; ``tile`` = n: the per-pose tensors repeated n times."""
    def c(v, per_pose=True):
        if v is None:
            return None
        v = torch.as_tensor(v).to(dtype)
        return v.repeat((tile,) + (1,) * (v.dim() - 1)) if (tile and per_pose) else v
    return dict(mode=q["mode"], a=c(q["a"], False), b=c(q["b"], False), root=c(q["root"]), transl=c(q["cam"]), j_rest=c(_jrest(), False), kp=c(q["kp"]),
                conf=c(q["conf"]), rows=q["rows"], focal=c(q["focal"]), center=c(q["center"]), sigma=q["sigma"], z_near=q["z_near"])


def _lib_stage(bm, q, y0, **over):
    from dposer_amd.tasks.completion import keypoint_residual_stage
    q = dict(q, **over)
    dv = lambda v: None if v is None else _dev(v)
    return keypoint_residual_stage(bm, _normalizer(q["norm_kind"]), _dev(y0), _dev(q["kp"]), keypoints_conf=dv(q["conf"]), obs_joints=q["rows"],
                                   cam_t=_dev(q["cam"]), camera_center=_dev(q["center"]), focal_length=_dev(q["focal"]), sigma=q["sigma"],
                                   z_near=q["z_near"], root_orient=_dev(q["root"]))


def _stage_check(bm, q, y0, tag):
    """The library's (s, v) at y0: same bits twice, finite, exact zeros without a live entry, and max(STAGE_FLOOR, K_STAGE e32) against
    the float64 rule.  Returns (e_lib / e32 of s, of v) where defined."""
    s, v = _lib_stage(bm, q, y0)
    s2, v2 = _lib_stage(bm, q, y0)
    assert torch.equal(s, s2) and torch.equal(v, v2)                                   # the same bits
    ws, wv, live = kg.keypoint_stage(torch.tensor(y0, dtype=torch.float64), **_rule_kw(q))
    s32, v32, live32 = kg.keypoint_stage(torch.tensor(y0, dtype=torch.float32), **_rule_kw(q, torch.float32))
    assert torch.equal(live, live32)
    s, v, ws, wv = t2n(s).astype(np.float64), t2n(v).astype(np.float64), ws.numpy(), wv.numpy()
    assert np.isfinite(s).all() and np.isfinite(v).all()                               # NaN under dead entries never enters a sum
    dead_rows = ~live.any(dim=1).numpy()
    assert not s[dead_rows].any() and not v[dead_rows].any()                           # no live entry: exact zeros
    if dead_rows.all():
        return None
    es, ev = rel_err(s, ws), rel_err(v, wv)
    es32, ev32 = rel_err(s32.double().numpy(), ws), rel_err(v32.double().numpy(), wv)
    rs_, rv_ = es / max(es32, U32), ev / max(ev32, U32)                                # (a single pose's e32 can be 0 by luck: floored at U32)
    print(f"keypoint stage {tag}: s e_lib {es:.2e} e32 {es32:.2e} ratio {rs_:.2f} | v e_lib {ev:.2e} e32 {ev32:.2e} ratio {rv_:.2f}")
    _log_measured(f"keypoint stage {tag} | s ratio", rs_)
    _log_measured(f"keypoint stage {tag} | v ratio", rv_)
    assert max(rs_, rv_) <= 8.0, (tag, rs_, rv_)                                       # the same fp32 arithmetic in another order: more would be a bug
    assert es <= max(STAGE_FLOOR, K_STAGE * es32), (tag, es, es32)
    assert ev <= max(STAGE_FLOOR, K_STAGE * ev32), (tag, ev, ev32)
    return rs_, rv_


# ---- the stage alone -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_obs", [1, 3, 22])
@pytest.mark.parametrize("B", [1, 5, 65, 300])
def test_stage_against_the_rule(bm, B, n_obs):
    for conf_kind in ("none", "zeros", "row dead"):
        for norm_kind, sigma, focal in (("zscore", 100.0, 5000.0), ("minmax", 0.0, 1000.0), ("zscore", 0.0, 5000.0), ("minmax", 100.0, 1000.0)):
            q = _problem(B, n_obs, conf_kind, 100 * B + n_obs, norm_kind=norm_kind, focal=focal, sigma=sigma)
            y0 = np.random.RandomState(B + n_obs).standard_normal((B, 63)).astype(np.float32) * (1.0 if norm_kind == "zscore" else 0.5)
            _stage_check(bm, q, y0, f"B={B} n_obs={n_obs} {norm_kind} {conf_kind} sigma={sigma:g} f={focal:g}")


def test_joints_behind_the_near_plane_are_dead(bm):
    """cam_t z = 0.3 m: the camera stands inside the body and some joints lie at or behind z_near = 0.1.  The library's live set is the
    rule's: a NaN keypoint under such a joint (positive confidence) changes nothing, the result is bit for bit the one with those
    confidences set to 0, and s, v meet the rule -- which a joint wrongly dropped or wrongly kept would not."""
    B = 65
    q = _problem(B, 22, "zeros", 9, cam_z=(0.3, 0.3))
    y0 = np.random.RandomState(10).standard_normal((B, 63)).astype(np.float32)
    _, live, J = kg.stage_terms(torch.tensor(y0, dtype=torch.float64), **_rule_kw(q))
    Z = J[..., 2].numpy()
    behind = Z <= q["z_near"]
    conf_live = q["conf"] > 0
    assert (behind & conf_live).sum() >= 5 and (~behind & conf_live).sum() >= 100, (int((behind & conf_live).sum()), int((~behind & conf_live).sum()))
    assert np.abs(Z - q["z_near"]).min() > 1e-4                                            # no joint so near the plane that fp32 decides otherwise
    assert np.array_equal(live.numpy(), conf_live & ~behind)
    _stage_check(bm, q, y0, "near plane")
    s, v = _lib_stage(bm, q, y0)
    kp_nan = q["kp"].copy()
    kp_nan[behind] = np.nan
    s1, v1 = _lib_stage(bm, q, y0, kp=kp_nan)
    conf0 = q["conf"].copy()
    conf0[behind] = 0.0
    s2, v2 = _lib_stage(bm, q, y0, kp=kp_nan, conf=conf0)
    assert torch.isfinite(s1).all() and torch.isfinite(v1).all()
    assert torch.equal(s, s1) and torch.equal(v, v1) and torch.equal(s, s2) and torch.equal(v, v2)


# ---- the sampler -------------------------------------------------------------------------------------------------------------------------------
def _sampler_inputs(B, seed, n_run, n_obs=22, conf_kind="zeros", **kw):
    rs = np.random.RandomState(seed)
    q = _problem(B, n_obs, conf_kind, seed + 1, **kw)
    q["x0"] = rs.standard_normal((B, 63)).astype(np.float32)
    q["noise"] = rs.standard_normal((n_run, 1, B, 63)).astype(np.float32)
    return q


def _run(m, bm, kind, N, q, *, norm, grad_step=None, noise=True, seed=0, start_step=0, run_steps=-1, stride=1, x0=None, rows_slice=None):
    from dposer_amd.algorithms.advanced import sampling
    sde = _sde(kind, N)
    sl = (lambda v: v) if rows_slice is None else (lambda v: None if v is None else v[rows_slice])
    dv = lambda v: None if v is None else _dev(v)
    nz = q["noise"] if noise is True else noise
    grad_step = _gs(q["focal"][0]) if grad_step is None else grad_step
    if nz is not None and rows_slice is not None:
        nz = nz[:, :, rows_slice]
    return sampling.fused_keypoint_guided_sample(m, sde, _dev(sl(q["x0"]) if x0 is None else x0), torch.linspace(sde.T, 1e-3, N), bm,
                                                 _normalizer(q["norm_kind"]), _dev(sl(q["kp"])), keypoints_conf=dv(sl(q["conf"])), obs_rows=q["rows"],
                                                 cam_t=_dev(sl(q["cam"])), camera_center=_dev(sl(q["center"])), focal=_dev(sl(q["focal"])),
                                                 sigma=q["sigma"], z_near=q["z_near"], root_orient=dv(sl(q["root"])), norm=norm, grad_step=grad_step,
                                                 start_step=start_step, run_steps=run_steps, noise=dv(nz), seed=seed, traj_stride=stride)


def _rule_loop(p, kind, N, q, x_init, noise, *, norm, **kw):
    out = kg.keypoint_guided_loop(p, G.oracle_sde(kind, N), torch.as_tensor(x_init, dtype=torch.float64), noise, _rule_kw(q), norm=norm,
                                  grad_step=_gs(q["focal"][0]), **kw)
    assert out[3] > 1.0, out[3]                                                            # depth never decided liveness
    return out[:3]


def forced_errors(bm, kind, norm, prec, every, forward=False):
    """Teacher-forced whole grid, N = 1000, B = 5: (indices, t, e_lib, e32) -- every listed index stepped by the rule in float64 and in
    float32 from the library's own state after the index before (all indices side by side in one evaluation of the rule)."""
    N, B = 1000, 5
    cfg, m, p = _model(33, prec)
    q = _sampler_inputs(B, 71, N, focal=5000.0 if kind == "subvp" else 1000.0)
    traj, x, x_mean = _run(m, bm, kind, N, q, norm=norm)
    assert torch.isfinite(traj).all() and torch.equal(x, traj[-1])
    got = t2n(traj)
    idx = np.arange(0, N, every)
    n = len(idx)
    states = np.concatenate([q["x0"][None], got[:-1]])[idx].reshape(n * B, 63)
    ts = torch.linspace(1.0, 1e-3, N)
    out = {}
    for dt in (torch.float64, torch.float32):
        t = ts.to(dt)[idx].repeat_interleave(B)
        z = torch.as_tensor(q["noise"][idx, 0].reshape(n * B, 63)).to(dt)
        xs, xm, _, zmin = kg.keypoint_guided_step(G.params_as(p, dt), G.oracle_sde(kind, N), torch.as_tensor(states).to(dt), t, z, _rule_kw(q, dt, tile=n),
                                                  norm=norm, grad_step=_gs(q["focal"][0]), group=B)
        assert zmin > 1.0, zmin
        out[dt] = (xs.double().numpy().reshape(n, B, 63), xm.double().numpy().reshape(n, B, 63))
    want = out[torch.float64][0]
    e_lib = np.array([rel_err(got[i], want[k]) for k, i in enumerate(idx)])
    e32 = np.array([rel_err(out[torch.float32][0][k], want[k]) for k in range(n)])
    if not forward:
        return idx, ts.numpy()[idx], e_lib, e32
    # the float64 rule stepped on the LIBRARY's forward at the same states (values substituted, the Jacobian the rule's own)
    from dposer_amd.algorithms.advanced import utils as mutils
    from oracle import score_ref as R
    t64 = ts.double()[idx].repeat_interleave(B)
    m.eval()
    with torch.no_grad():
        s_lib = mutils.get_score_fn(_sde(kind, N), m, train=False, continuous=True)(_dev(states), _dev(t64.numpy()))
    s_lib = torch.as_tensor(t2n(s_lib).astype(np.float64))
    p64, x64 = G.params_as(p, torch.float64), torch.as_tensor(states).double()
    s_rule = R.score_fn(p64, G.oracle_sde(kind, N), x64, t64).detach()
    e_score = np.array([rel_err(s_lib[k * B:(k + 1) * B].numpy(), s_rule[k * B:(k + 1) * B].numpy()) for k in range(n)])
    z64 = torch.as_tensor(q["noise"][idx, 0].reshape(n * B, 63)).double()
    xs, _, _, _ = kg.keypoint_guided_step(p64, G.oracle_sde(kind, N), x64, t64, z64, _rule_kw(q, torch.float64, tile=n), norm=norm,
                                          grad_step=_gs(q["focal"][0]), group=B, score_shift=s_lib - s_rule)
    on_fwd = xs.numpy().reshape(n, B, 63)
    e_fwd = np.array([rel_err(on_fwd[k], want[k]) for k in range(n)])                       # what the forward's error alone does to the step
    e_res = np.array([rel_err(got[i], on_fwd[k]) for k, i in enumerate(idx)])               # the library against the rule on its own forward
    return idx, ts.numpy()[idx], e_lib, e32, e_fwd, e_res, e_score


@pytest.mark.parametrize("prec,every", [("fp32", 10), ("bf16x3", 10), ("bf16", 50)])
@pytest.mark.parametrize("norm", ["sample", "batch"])
@pytest.mark.parametrize("kind", ["subvp", "vp"])
def test_every_tenth_index_of_a_whole_run_against_the_float64_rule(bm, kind, norm, prec, every):
    idx, t, e_lib, e32, *fwd = forced_errors(bm, kind, norm, prec, every, forward=prec == "bf16x3")
    assert np.isfinite(e_lib).all()
    tol = STEP_TOLS[prec]
    if prec == "bf16":
        late = t <= 0.2
        print(f"{kind} {norm} bf16: worst rel-L2 {e_lib[late].max():.2e} over t <= 0.2 (bound {tol:.0e}), {e_lib[~late].max():.2e} over the rest")
        assert e_lib[late].max() <= tol
        return
    err = e_lib                                                         # what is held to max(STEP_TOLS, K e32)
    if prec == "bf16x3":                                                # (module docstring: the rule on the library's own forward)
        e_fwd, err, e_score = fwd
        print(f"{kind} {norm} bf16x3: forward rel-L2 per index at most {e_score.max():.2e}; against the plain rule worst e_lib / e32 "
              f"{float((e_lib / e32)[(e32 > tol) | (e_lib > tol)].max()):.2f}, worst e_lib / (e_fwd + e32) {float((e_lib / (e_fwd + e32)).max()):.2f}")
        assert e_score.max() <= tol, e_score.max()                      # the forward itself: a score is one step's worth of accuracy
    bound = np.maximum(tol, K_E32[prec] * e32)
    branch = np.nonzero(bound > tol)[0]                                 # decided by the e32 branch
    first = 0 if len(branch) == 0 else int(branch[-1]) + 1              # from here on the bound is STEP_TOLS alone
    over = np.nonzero((e32 > tol) | (err > tol))[0]                     # every index the e32 branch has to decide
    ratio = float((err[over] / e32[over]).max()) if len(over) else 0.0
    print(f"{kind} {norm} {prec}: {100.0 * len(branch) / len(idx):.1f} % of the indices decided by the e32 branch, STEP_TOLS alone from index "
          f"{int(idx[first]) if first < len(idx) else 'none'}, worst error / e32 where e32 or the error > STEP_TOLS {ratio:.2f}, worst error {err.max():.2e}, "
          f"worst error from that index on {err[first:].max() if first < len(idx) else 0.0:.2e}")
    _log_measured(f"keypoint sampler {kind} {norm} {prec} | worst error / e32", ratio)
    assert ratio <= 8.0, ratio                                          # the same fp32 arithmetic in another order: more would be a bug
    bad = np.nonzero(err > bound)[0]
    assert len(bad) == 0, [(int(idx[k]), float(err[k]), float(e32[k])) for k in bad[:10]]


def test_a_row_does_not_depend_on_its_batch_mates(bm):
    """norm="sample": rows [0:2] of a B = 5 call against the two rows run alone, under injected noise: the same bits.  The batch scope does
    couple the rows."""
    N, B, start = 12, 5, 6
    cfg, m, p = _model(33, "fp32")
    q = _sampler_inputs(B, 81, N - start)
    big, _, _ = _run(m, bm, "subvp", N, q, norm="sample", start_step=start)
    two, _, _ = _run(m, bm, "subvp", N, q, norm="sample", start_step=start, rows_slice=slice(0, 2))
    assert torch.isfinite(big).all() and torch.equal(big[:, 0:2], two)
    big_b, _, _ = _run(m, bm, "subvp", N, q, norm="batch", start_step=start)
    assert rel_err(t2n(big_b[-1, 0:2]), t2n(two[-1])) > 1e-3


def test_no_live_entry_and_zero_grad_step_are_the_plain_sampler(bm):
    from dposer_amd.algorithms.advanced import sampling
    N, B, seed = 40, 65, 12345
    cfg, m, p = _model(35, "fp32")
    q = _sampler_inputs(B, 73, N, conf_kind="row dead")
    sde = _sde("subvp", N)
    _, b, bmean = sampling.fused_em_sample(m, sde, _dev(q["x0"]), torch.linspace(sde.T, 1e-3, N), seed=seed)      # same Philox stream and index
    _, a, am = _run(m, bm, "subvp", N, q, norm="sample", grad_step=0.0, noise=None, seed=seed)
    e, em = rel_err(t2n(a), t2n(b)), rel_err(t2n(am), t2n(bmean))
    print(f"grad_step = 0 vs dposer_em_sampler: x {e:.2e}, x_mean {em:.2e}")
    assert e < TOLS["fp32"] and em < TOLS["fp32"]
    _, c, cm = _run(m, bm, "subvp", N, q, norm="sample", noise=None, seed=seed)                                  # row 0 has no live entry
    assert torch.equal(c[0], a[0]) and torch.equal(cm[0], am[0]) and not torch.equal(c[1], a[1])
    e0 = rel_err(t2n(c[0]), t2n(b[0]))
    print(f"a row without a live entry vs dposer_em_sampler: {e0:.2e}")
    assert e0 < TOLS["fp32"]
    q2 = dict(q, conf=np.zeros_like(q["conf"]))                                                                 # no live entry anywhere: batch scope too
    _, d, _ = _run(m, bm, "subvp", N, q2, norm="batch", noise=None, seed=seed)
    assert torch.equal(d, a)


@pytest.mark.parametrize("norm", ["sample", "batch"])
def test_repeated_split_and_strided_runs_give_the_same_bits(bm, norm):
    N, k, B = 32, 13, 65
    cfg, m, p = _model(35, "fp32")
    q = _sampler_inputs(B, 74, N, focal=1000.0)
    for kw in (dict(noise=q["noise"]), dict(noise=None, seed=99)):
        a = _run(m, bm, "vp", N, q, norm=norm, **kw)
        b = _run(m, bm, "vp", N, q, norm=norm, **kw)
        for u, v in zip(a, b):
            assert torch.isfinite(u).all() and torch.equal(u, v)
        head = dict(kw, noise=None if kw["noise"] is None else kw["noise"][:k])
        tail = dict(kw, noise=None if kw["noise"] is None else kw["noise"][k:])
        t1, x1, _ = _run(m, bm, "vp", N, q, norm=norm, run_steps=k, **head)
        t2, x2, xm2 = _run(m, bm, "vp", N, q, norm=norm, start_step=k, x0=t2n(x1), **tail)
        assert t1.shape == (k, B, 63) and torch.equal(torch.cat([t1, t2]), a[0]) and torch.equal(x2, a[1]) and torch.equal(xm2, a[2])
        s4 = _run(m, bm, "vp", N, q, norm=norm, stride=4, **kw)
        assert s4[0].shape == (N // 4, B, 63) and torch.equal(s4[0], a[0][3::4]) and torch.equal(s4[1], a[1])
    c = _run(m, bm, "vp", N, q, norm=norm, noise=None, seed=100)
    assert not torch.equal(c[1], a[1])


@pytest.mark.parametrize("B", [65, 1])
def test_ragged_and_single_row_batches_free_running(bm, B):
    """N = 12 from start_step = 6 (t <= 0.5), free-running against the rule."""
    N, start = 12, 6
    cfg, m, p = _model(33, "fp32")
    for norm, n_obs, focal, norm_kind in (("sample", 22, 5000.0, "zscore"), ("batch", 3, 1000.0, "minmax")):
        q = _sampler_inputs(B, 72 + B, N - start, n_obs=n_obs, conf_kind="zeros" if B > 1 else "none", focal=focal, norm_kind=norm_kind)
        traj, x, x_mean = _run(m, bm, "subvp", N, q, norm=norm, start_step=start)
        want, wx, wm = _rule_loop(p, "subvp", N, q, q["x0"], q["noise"], norm=norm, start_step=start)
        errs = [rel_err(a, b) for a, b in zip(t2n(traj), want.numpy())] + [rel_err(t2n(x_mean), wm.numpy())]
        print(f"B = {B} {norm}: worst rel-L2 {max(errs):.2e}")
        assert max(errs) < TOLS["fp32"]


class _Counting:
    def __init__(self, lib, calls):
        self._lib, self._calls = lib, calls

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*a):
            self._calls.append(name)
            return fn(*a)

        return call


class _Wrapped(torch.nn.Module):
    """The same network behind a module that is not a ScoreModelFC: the pair the one-call path does not take."""

    def __init__(self, inner):
        super().__init__()
        self.inner = inner

    def forward(self, x, labels, condition=None, mask=None):
        return self.inner(x, labels)


def test_the_supported_pair_is_one_library_call_and_the_stepwise_path_agrees(bm, monkeypatch):
    from dposer_amd.algorithms.advanced import sampling
    N, B = 20, 8
    cfg, m, p = _model(36, "fp32")
    start = 10                                                                 # free-running: from t <= 0.5
    q = _sampler_inputs(B, 75, N - start, n_obs=3)
    fn = sampling.get_keypoint_guided_sampler(_sde("subvp", N), (B, 63), bm, _normalizer("zscore"), focal_length=5000.0, sigma=q["sigma"],
                                              z_near=q["z_near"], grad_step=_gs(5000.0), norm="sample", denoise=False, device=DEV)
    kw = dict(keypoints_conf=_dev(q["conf"]), obs_joints=q["rows"], cam_t=_dev(q["cam"]), camera_center=_dev(q["center"]), root_orient=_dev(q["root"]),
              z=_dev(q["x0"]), start_step=start, noise=_dev(q["noise"]))
    eng = m._engine()
    eng.packed(m.flat_params(), with_backward=True, force=True)
    bm.fk_joints(torch.zeros(1, 63, device=DEV))                               # the body handle exists
    m.freeze_packed, keep = True, m.freeze_packed
    calls = []
    monkeypatch.setattr(eng, "lib", _Counting(eng.lib, calls))
    m.train()
    try:
        trajs, x = fn(m, _dev(q["kp"]), **kw)
        assert m.training
    finally:
        m.eval()
        m.freeze_packed = keep
        monkeypatch.undo()
    heavy = [c for c in calls if any(s in c for s in ("sampler", "forward", "backward", "langevin", "prior", "dsm", "stage", "fk_"))]
    assert heavy == ["dposer_keypoint_guided_sampler"], calls
    assert all(t.grad is None for t in m.parameters())
    assert trajs.shape == (N - start, B, 63) and torch.equal(x, trajs[-1])
    # a model outside the one-call path: the step-by-step loop with torch autograd through the model and fk_joints(grad="chain")
    t2, x2 = fn(_Wrapped(m), _dev(q["kp"]), **kw)
    e = max(rel_err(t2n(a), t2n(b)) for a, b in zip(t2, trajs))
    print(f"step-by-step loop vs one call, worst index rel-L2 {e:.2e}")
    assert e < TOLS["fp32"] and all(t.grad is None for t in m.parameters())


def test_a_nan_keypoint_under_a_positive_confidence_raises_after_the_loop(bm):
    from dposer_amd.algorithms.advanced import sampling
    N, B = 12, 8
    cfg, m, p = _model(36, "fp32")
    q = _sampler_inputs(B, 76, N, conf_kind="none")
    kp = q["kp"].copy()
    kp[2, 5, 1] = np.nan
    fn = sampling.get_keypoint_guided_sampler(_sde("subvp", N), (B, 63), bm, _normalizer("zscore"), grad_step=GRAD_STEP, device=DEV)
    kw = dict(cam_t=_dev(q["cam"]), camera_center=_dev(q["center"]), root_orient=_dev(q["root"]), z=_dev(q["x0"]), noise=_dev(q["noise"]))
    with pytest.raises(ValueError, match=r"Consider reduce the value of parameter: grad_step=0\.7.*index 0\b"):
        fn(m, _dev(kp), **kw)
    assert not m.training
    trajs, x = fn(m, _dev(q["kp"]), **kw)                                      # the next call is unaffected
    assert torch.isfinite(trajs).all()
    with pytest.raises(ValueError, match="distinct"):                          # host checks come before any device work
        fn(m, _dev(q["kp"][:, :2]), obs_joints=[4, 4], **kw)
    with pytest.raises(ValueError, match=r"\[0, 22\)"):
        fn(m, _dev(q["kp"][:, :2]), obs_joints=[4, 22], **kw)


def test_sample_from_keypoints(bm):
    """B = 3 observations, 4 hypotheses each, N = 50: shapes, the reprojection error formula against numpy, mpjpe = the minimum over a
    direct pose_pair_errors call.  Whether guidance lowers the reprojection error cannot be asserted with random weights: printed."""
    from dposer_amd.tasks.completion import sample_from_keypoints
    from dposer_amd.utils.metric import pose_pair_errors
    N, B, K, start = 50, 3, 4, 25
    cfg, m, p = _model(33, "fp32")
    nz = _normalizer("zscore")
    sde = _sde("subvp", N)
    q = _problem(B, 22, "zeros", 5, focal=1000.0)
    rs = np.random.RandomState(6)
    gt = nz.offline_denormalize(_dev(rs.standard_normal((B, 63)) * 0.5))
    z = _dev(rs.standard_normal((B * K, 63)))
    noise = _dev(rs.standard_normal((N, 1, B * K, 63)))[start:]
    kw = dict(keypoints_conf=_dev(q["conf"]), cam_t=_dev(q["cam"]), camera_center=_dev(q["center"]), focal_length=1000.0, root_orient=_dev(q["root"]),
              hypo=K, noise=noise, z=z, start_step=start)
    out = sample_from_keypoints(m, sde, nz, bm, _dev(q["kp"]), grad_step=0.2 * 4.0 / 1000.0, gt_poses=gt, **kw)         # test_sample_from_joints' 0.2, in pixels
    assert out["poses"].shape == (B, K, 63) and out["reprojection_error"].shape == (B, K) and out["depth_spread"].shape == (B,)
    assert out["mpjpe"].shape == (B,) and out["mpvpe"].shape == (B,)
    assert bool(torch.isfinite(out["poses"]).all()) and bool(torch.isfinite(out["mpjpe"]).all()) and bool((out["depth_spread"] > 0).all())
    # the formula, in numpy float64 from the returned poses
    poses = t2n(out["poses"]).astype(np.float64).reshape(B * K, 63)
    rep = lambda v: np.repeat(v, K, axis=0)
    J = jg.fk22(torch.tensor(poses), torch.tensor(rep(q["root"])).double(), torch.tensor(_jrest()), torch.tensor(rep(q["cam"])).double()).numpy()
    live = rep(q["conf"] > 0) & (J[..., 2] > q["z_near"])
    proj = 1000.0 * J[..., :2] / J[..., 2:3] + np.array(CENTER)
    dist = np.sqrt(((proj - np.where(live[..., None], rep(q["kp"]), 0.0)) ** 2).sum(axis=2))
    want = np.array([dist[i][live[i]].mean() if live[i].any() else np.nan for i in range(B * K)]).reshape(B, K)
    got = t2n(out["reprojection_error"])
    assert np.allclose(got, want, rtol=1e-4, atol=1e-2, equal_nan=True), (got, want)     # fp32 pixels of a few hundred: 1e-2 px
    depth = J[..., 2].mean(axis=1).reshape(B, K)
    assert np.allclose(t2n(out["depth_spread"]), depth.std(axis=1), rtol=1e-3, atol=1e-5)
    pe = pose_pair_errors(bm, gt, out["poses"], per_hypothesis=True)
    assert pe["mpjpe_h"].shape == (B, K)
    assert torch.equal(out["mpjpe"], pe["mpjpe_h"].min(dim=1).values) and torch.equal(out["mpvpe"], pe["mpvpe_h"].min(dim=1).values)
    base = sample_from_keypoints(m, sde, nz, bm, _dev(q["kp"]), grad_step=0.0, **kw)                             # unconditional, the same draws
    print(f"mean reprojection error: guided {float(out['reprojection_error'].nanmean()):.1f} px, unconditional "
          f"{float(base['reprojection_error'].nanmean()):.1f} px; depth spread guided {t2n(out['depth_spread'])}, unconditional {t2n(base['depth_spread'])}")
