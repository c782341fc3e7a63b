"""GPU tests of dposer_pose_pair_errors through utils.metric.pose_pair_errors, Evaler(fused=True) and the raw C ABI: against the
reference's own evaluator (golden g18), against the float64 rule of tests/pair_err_ref.py over a sweep of shapes, and the exactness
properties the header promises (a sample's outputs are a function of its own data; minimum with torch.min's NaN rule)."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

import pair_err_ref
from gpu_common import DEV, t2n
from helpers import load

pytestmark = pytest.mark.gpu

KEYS = ("mpvpe", "mpjpe", "mpvpe_h", "mpjpe_h")


@pytest.fixture(scope="module")
def full():
    from dposer_amd.body_model.body_model import BodyModel
    from dposer_amd.body_model.synthetic import make_synthetic_smplx_asset
    return BodyModel(make_synthetic_smplx_asset(seed=0)).to(DEV)


@pytest.mark.parametrize("part", pair_err_ref.PARTS)
def test_fused_evaler_matches_the_reference_evaluator(part, full):
    """Evaler(fused=True) against g18 (the reference's own Evaler, B = 6, H = 3) under the bound the unfused path is held to
    (2e-5 of the largest value; measured 1.3e-7 .. 1.1e-6 over the nine parts)."""
    from dposer_amd.dataset.AMASS import Evaler
    g = load("g18_evaler")
    ev = Evaler(full, part=part)
    outs, gts = torch.tensor(g["outs"], device=DEV), torch.tensor(g["gts"], device=DEV)
    tag = part or "all"
    r = ev.multi_eval_bodys(outs, gts, fused=True)
    rt = ev.multi_eval_bodys(outs, gts, as_tensors=True, fused=True)
    r0 = ev.eval_bodys(outs[:, 0].contiguous(), gts, fused=True)
    assert set(r) == set(r0) == {"mpvpe_all", "mpjpe_body"}
    for k in ("mpvpe_all", "mpjpe_body"):
        assert isinstance(r[k], np.ndarray) and r[k].shape == (6,) and rt[k].is_cuda and np.array_equal(t2n(rt[k]), r[k])
        e = np.abs(r[k] - g[f"{tag}/{k}"]).max() / np.abs(g[f"{tag}/{k}"]).max()
        e0 = np.abs(t2n(r0[k]) - g[f"{tag}/h0_{k}"]).max() / np.abs(g[f"{tag}/h0_{k}"]).max()
        print(f"g18 {tag} {k}: fused {e:.2e}, first hypothesis {e0:.2e}")
        assert e < 2e-5 and e0 < 2e-5, (part, k, e, e0)
    alone = ev.multi_eval_bodys(outs[2:3].contiguous(), gts[2:3].contiguous(), as_tensors=True, fused=True)      # (the 1024-entry form of the kernel too)
    for k in ("mpvpe_all", "mpjpe_body"):
        assert np.array_equal(t2n(alone[k]).view(np.int32), t2n(rt[k][2:3]).view(np.int32)), (part, k)


# ---- shape sweep against the float64 rule --------------------------------------------------------------------------------------
V_SMALL, B_MAX, H_MAX = 1100, 130, 3
_CASES = {}


def _case(nnz, per_sample_betas):
    """Model, inputs and the float64 bodies of the LARGEST case (B = 130, H = 3) of one (ELL width, betas mode); smaller cases are
    its leading samples / hypotheses (a sample's reference does not depend on the batch).  Built once, never modified."""
    key = (nnz, per_sample_betas)
    if key not in _CASES:
        from dposer_amd.body_model.body_model import BodyModel
        from dposer_amd.body_model.synthetic import make_synthetic_smplx_asset
        asset = make_synthetic_smplx_asset(seed=7 + nnz, num_vertices=V_SMALL, nnz_per_vertex=nnz)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)          # (width 5: "the general LBS kernels are used")
            bm = BodyModel(asset).to(DEV)
        rs = np.random.RandomState(100 + nnz)
        ref = (rs.standard_normal((B_MAX, 63)) * 0.3).astype(np.float32)
        hyp = (ref[:, None] + rs.standard_normal((B_MAX, H_MAX, 63)) * 0.1).astype(np.float32)
        betas = (rs.standard_normal((B_MAX, 10)) * 0.5).astype(np.float32) if per_sample_betas else None
        vr, jr = pair_err_ref.bodies(asset, ref, betas)
        vh, jh = zip(*[pair_err_ref.bodies(asset, hyp[:, h], betas) for h in range(H_MAX)])
        _CASES[key] = dict(asset=asset, bm=bm, ref=ref, hyp=hyp, betas=betas, vr=vr, jr=jr, vh=vh, jh=jh)
    return _CASES[key]


def _lists(name):
    if name == "all":
        return None, None
    if name == "scattered":
        return np.array([V_SMALL - 1, 0, 3, 700, 257, 256, 255, 1024, 19, 511] + list(range(40, 1000, 3))), np.array([126, 0, 54, 55, 75, 76, 21, 100])
    return np.array([777]), np.array([90])                           # one vertex, one (landmark) row


def _want(c, B, H, vi, ji, scale):
    sel = lambda x, idx: x[:B] if idx is None else x[:B][:, idx]
    ev = np.stack([np.sqrt(((sel(c["vh"][h], vi) - sel(c["vr"], vi)) ** 2).sum(-1)).mean(-1) * scale for h in range(H)], 1)
    ej = np.stack([np.sqrt(((sel(c["jh"][h], ji) - sel(c["jr"], ji)) ** 2).sum(-1)).mean(-1) * scale for h in range(H)], 1)
    return {"mpvpe": ev.min(1), "mpjpe": ej.min(1), "mpvpe_h": ev, "mpjpe_h": ej}


def _unfused(bm, ref, hyp, betas, vi, ji, scale):
    """The evaluator's whole-mesh computation (two BodyModel.forward calls per hypothesis, torch reductions)."""
    ev, ej = [], []
    with torch.no_grad():
        for h in range(hyp.shape[1]):
            gt, out = bm(pose_body=ref, betas=betas), bm(pose_body=hyp[:, h].contiguous(), betas=betas)
            dv, dj = out.v - gt.v, out.Jtr - gt.Jtr
            if vi is not None:
                dv, dj = dv[:, torch.tensor(vi, device=DEV)], dj[:, torch.tensor(ji, device=DEV)]
            ev.append(torch.sqrt((dv ** 2).sum(-1)).mean(-1) * scale)
            ej.append(torch.sqrt((dj ** 2).sum(-1)).mean(-1) * scale)
    ev, ej = torch.stack(ev, 1), torch.stack(ej, 1)
    return {"mpvpe": ev.min(1).values, "mpjpe": ej.min(1).values, "mpvpe_h": ev, "mpjpe_h": ej}


def _err(got, want):
    return max(float(np.abs(t2n(got[k]).astype(np.float64) - want[k]).max() / np.abs(want[k]).max()) for k in KEYS)


@pytest.mark.parametrize("lists", ["all", "scattered", "one"])
@pytest.mark.parametrize("per_sample_betas", [False, True])
@pytest.mark.parametrize("nnz", [4, 5])
@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("B", [1, 5, 130])
def test_shape_sweep_against_the_float64_rule(B, H, nnz, per_sample_betas, lists):
    """B x H x ELL width (5 = the general loop) x shared / per-sample betas x three list choices on a 1100-vertex asset (five
    256-entry blocks, ragged tail; extras and landmarks wrap into range) against tests/pair_err_ref.py.  The tolerance is not fixed in
    advance: the fused result must lie within 1.5 x the error of the unfused evaluator computation (BodyModel.forward for both bodies +
    torch reductions) against the same float64 rule, or within 2e-5 relative, whichever is larger; the margin is the different
    summation order of a mean over at most 10475 fp32 terms.  Error = largest |x - rule| over the largest |rule|, worst of
    mpvpe / mpjpe and their per-hypothesis forms.
    Measured on an MI355X, largest error over the 72 cases (unfused / fused): all vertices and rows 4.93e-7 / 4.70e-7; scattered lists
    8.52e-7 / 8.64e-7; one vertex and one row 2.97e-6 / 2.97e-6 (no mean to average the rounding of a single fp32 vertex); largest
    fused / unfused ratio of one case 2.3, both sides below 1e-6 there -- every case sits under the 2e-5 floor."""
    from dposer_amd.utils.metric import pose_pair_errors
    c = _case(nnz, per_sample_betas)
    vi, ji = _lists(lists)
    scale = 1000.0
    ref, hyp = torch.tensor(c["ref"][:B], device=DEV), torch.tensor(c["hyp"][:B, :H], device=DEV)
    betas = None if c["betas"] is None else torch.tensor(c["betas"][:B], device=DEV)
    want = _want(c, B, H, vi, ji, scale)
    got = pose_pair_errors(c["bm"], ref, hyp, vert_idx=vi, joint_idx=ji, scale=scale, betas=betas, per_hypothesis=True)
    assert got["mpvpe"].shape == (B,) and got["mpjpe_h"].shape == (B, H) and all(got[k].is_cuda and got[k].dtype == torch.float32 for k in KEYS)
    e_fused, e_unfused = _err(got, want), _err(_unfused(c["bm"], ref, hyp, betas, vi, ji, scale), want)
    print(f"sweep B={B} H={H} nnz={nnz} betas={'per-sample' if per_sample_betas else 'shared'} lists={lists}: unfused {e_unfused:.3e} fused {e_fused:.3e}")
    assert e_fused <= max(1.5 * e_unfused, 2e-5), (e_fused, e_unfused)


# ---- exactness ---------------------------------------------------------------------------------------------------------------------
def _bits(r, keys=("mpvpe", "mpjpe")):
    return [t2n(r[k]).view(np.int32) for k in keys]


def test_a_hypothesis_equal_to_its_reference_scores_exactly_zero():
    from dposer_amd.utils.metric import pose_pair_errors
    for nnz in (4, 5):
        c = _case(nnz, True)
        ref = torch.tensor(c["ref"][:5], device=DEV)
        hyp = torch.tensor(c["hyp"][:5], device=DEV).clone()
        hyp[:, 1] = ref
        r = pose_pair_errors(c["bm"], ref, hyp, scale=1000.0, betas=torch.tensor(c["betas"][:5], device=DEV), per_hypothesis=True)
        for k in ("mpvpe", "mpjpe"):
            assert np.array_equal(t2n(r[k]), np.zeros(5, np.float32)) and np.array_equal(t2n(r[k + "_h"][:, 1]), np.zeros(5, np.float32))
            assert (t2n(r[k + "_h"][:, 0]) > 0).all()


def test_a_sample_carries_its_own_bits_whatever_the_batch():
    """Sample k of a batch of 130 = the same sample alone = the same sample at another position; hypotheses split into groups by a small
    workspace budget, and hypotheses permuted, change no bit; the per-hypothesis outputs reduce to the minima exactly."""
    from dposer_amd import _C
    from dposer_amd.utils.metric import pose_pair_errors
    c = _case(4, True)
    vi, ji = _lists("scattered")
    ref, hyp, betas = (torch.tensor(c[k], device=DEV) for k in ("ref", "hyp", "betas"))
    for lists in (dict(), dict(vert_idx=vi, joint_idx=ji)):
        whole = pose_pair_errors(c["bm"], ref, hyp, betas=betas, scale=1000.0, per_hypothesis=True, **lists)
        for k in (0, 77, 129):
            alone = pose_pair_errors(c["bm"], ref[k:k + 1], hyp[k:k + 1], betas=betas[k:k + 1], scale=1000.0, per_hypothesis=True, **lists)
            for key in KEYS:
                assert np.array_equal(t2n(alone[key]).view(np.int32), t2n(whole[key][k:k + 1]).view(np.int32)), (k, key)
        perm = torch.tensor(np.random.RandomState(3).permutation(B_MAX), device=DEV)
        moved = pose_pair_errors(c["bm"], ref[perm], hyp[perm], betas=betas[perm], scale=1000.0, per_hypothesis=True, **lists)
        for key in KEYS:
            assert np.array_equal(t2n(moved[key]).view(np.int32), t2n(whole[key][perm]).view(np.int32)), key
        # groups: a budget that holds the front workspace of 130 x 2 poses but not of 130 x 3
        lib, h = _C.lib(), c["bm"].bm._handle()
        budget = int(lib.dposer_lbs_workspace_bytes(h, B_MAX * 2))
        assert budget < lib.dposer_lbs_workspace_bytes(h, B_MAX * 3)
        for b in (budget, 1):                                        # groups of 2 + 1, and 1 + 1 + 1
            split = pose_pair_errors(c["bm"], ref, hyp, betas=betas, scale=1000.0, per_hypothesis=True, max_workspace_bytes=b, **lists)
            for key in KEYS:
                assert np.array_equal(t2n(split[key]).view(np.int32), t2n(whole[key]).view(np.int32)), (b, key)
        swapped = pose_pair_errors(c["bm"], ref, hyp[:, [2, 0, 1]].contiguous(), betas=betas, scale=1000.0, **lists)
        assert all(np.array_equal(a, b) for a, b in zip(_bits(swapped), _bits(whole)))
        for k in ("mpvpe", "mpjpe"):
            assert torch.equal(whole[k + "_h"].min(1).values, whole[k])


def test_a_nan_hypothesis_makes_only_its_sample_nan():
    from dposer_amd.utils.metric import pose_pair_errors
    c = _case(4, False)
    ref, hyp = torch.tensor(c["ref"][:5], device=DEV), torch.tensor(c["hyp"][:5], device=DEV)
    clean = pose_pair_errors(c["bm"], ref, hyp, scale=1000.0)
    bad = hyp.clone()
    bad[3, 1, 0] = float("nan")
    others = [0, 1, 2, 4]
    for budget in (1 << 30, 1):                                      # one call; three calls: the NaN arrives through min_into and is kept by the next
        r = pose_pair_errors(c["bm"], ref, bad, scale=1000.0, max_workspace_bytes=budget)
        for k in ("mpvpe", "mpjpe"):
            got = t2n(r[k])
            assert np.isnan(got[3]), (budget, k)
            assert np.array_equal(got[others].view(np.int32), t2n(clean[k])[others].view(np.int32)), (budget, k)
    first = bad[:, [1, 0, 2]].contiguous()                           # the NaN in the first group, finite values folded in afterwards
    r = pose_pair_errors(c["bm"], ref, first, scale=1000.0, max_workspace_bytes=1)
    assert np.isnan(t2n(r["mpvpe"])[3]) and np.isnan(t2n(r["mpjpe"])[3])


def test_evaluate_completion_with_the_fused_evaluator(full):
    """tasks/completion.evaluate_completion(fused_eval=True) at the sizes of test_evaluate_completion_end_to_end under the same seed: the same
    completions scored by the other evaluator -- per-sample values agree to ~1e-5, so their means to 1e-4."""
    from dposer_amd.algorithms.advanced import sde_lib
    from dposer_amd.dataset.AMASS import Posenormalizer
    from dposer_amd.tasks.completion import evaluate_completion
    from gpu_common import make_model
    cfg, m, p = make_model(64, precision="bf16")
    g = load("g10_normalizer")
    stats = {k.split("/")[-1]: torch.tensor(g[k]) for k in g.files if k.startswith("stats/axis_normalize")}
    nz = Posenormalizer(stats, device=DEV, normalize=True, min_max=False, rot_rep="axis")
    poses = torch.tensor(g["norm_minmax0"][:48])
    sde = sde_lib.subVPSDE(0.1, 20.0, 1000)
    kw = dict(iterations=1, steps_per_iter=3)
    res = {}
    for fused in (False, True):
        torch.manual_seed(5)
        res[fused] = evaluate_completion(m, sde, nz, full, poses, part="legs", hypo=2, batch_size=16, optimize_kwargs=kw, fused_eval=fused)
    (m0, n0), (m1, n1) = res[False], res[True]
    assert n0 == n1 == 48 and set(m0) == set(m1) == {"mpvpe_all", "mpjpe_body"}
    for k in m0:
        print(f"evaluate_completion {k}: unfused {m0[k]:.6f} fused {m1[k]:.6f}")
        assert abs(m1[k] - m0[k]) <= 1e-4 * abs(m0[k]), (k, m0[k], m1[k])


def test_the_c_entry_stays_inside_its_output_buffers():
    """dposer_pose_pair_errors through _C.lib() with a guard word behind every output: nothing is written past [B] / [B, H]."""
    from dposer_amd import _C
    c = _case(4, False)
    core = c["bm"].bm
    lib, h = _C.lib(), core._handle()
    B, H, G = 5, 3, 64
    ref = core.lbs_front(body_pose=torch.tensor(c["ref"][:B], device=DEV))
    hyp = core.lbs_front(body_pose=torch.tensor(c["hyp"][:B], device=DEV).reshape(B * H, 63))
    vi = torch.tensor(_lists("scattered")[0], dtype=torch.int32, device=DEV)
    outs = {k: torch.full((n + G,), -7.0, dtype=torch.float32, device=DEV) for k, n in (("mpvpe", B), ("mpjpe", B), ("mpvpe_h", B * H), ("mpjpe_h", B * H))}
    nbytes = int(lib.dposer_pose_pair_errors_scratch_bytes(h, B, H, len(vi)))
    scratch = torch.full((nbytes + 4096,), 0xAB, dtype=torch.uint8, device=DEV)
    a = _C.PosePairErrorsArgs(body=h, ws_ref=ref.ws.data_ptr(), ws_hyp=hyp.ws.data_ptr(), joints_ref=ref.joints.data_ptr(), joints_hyp=hyp.joints.data_ptr(),
                              v_shaped=ref.v_shaped.data_ptr(), v_shaped_batched=0, skin_k=4, skin_idx=core.skin_idx.data_ptr(), skin_w=core.skin_w.data_ptr(),
                              vert_list=vi.data_ptr(), num_listed_vertices=len(vi), hypotheses=H, extra_vertex_ids=core.extra_vertex_ids.data_ptr(),
                              lmk_tri=core.lmk_tri.data_ptr(), lmk_bary=core.lmk_bary_coords.data_ptr(), batch=B, scale=100.0, min_into=0,
                              mpvpe=outs["mpvpe"].data_ptr(), mpjpe=outs["mpjpe"].data_ptr(), mpvpe_h=outs["mpvpe_h"].data_ptr(),
                              mpjpe_h=outs["mpjpe_h"].data_ptr(), scratch=scratch.data_ptr())
    _C.check(lib.dposer_pose_pair_errors(C.byref(a), _C.stream_ptr()), "dposer_pose_pair_errors")
    torch.cuda.synchronize()
    for k, n in (("mpvpe", B), ("mpjpe", B), ("mpvpe_h", B * H), ("mpjpe_h", B * H)):
        assert bool((outs[k][n:] == -7.0).all()) and bool((outs[k][:n] > 0).all()), k
    assert bool((scratch[nbytes:] == 0xAB).all())
    want = _want(c, B, H, _lists("scattered")[0], None, 100.0)       # centimetres, all 127 joint rows
    assert np.abs(t2n(outs["mpvpe"][:B]) - want["mpvpe"]).max() / want["mpvpe"].max() < 2e-5
    assert np.abs(t2n(outs["mpjpe_h"][:B * H]).reshape(B, H) - want["mpjpe_h"]).max() / want["mpjpe_h"].max() < 2e-5
