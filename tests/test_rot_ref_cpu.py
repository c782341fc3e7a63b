"""CPU checks of the band machinery in tests/rot_ref.py: the conditions the band inputs must meet, the float32 yardsticks against the
existing hard caps, and eight planted errors -- deliberately wrong float32 statements of the rotation rules that must break the band
bound (4 x yardstick + floor) in a named band.  They show, without a GPU, that tests/test_gpu_rotations.py can fail.

Measured here (factor = error of the planted variant / the band bound it is held to):

    planted error                                          band         factor
    1 Rodrigues without the +1e-8 offset                   0            inf   (0 / 0)
    2 log map through acos and skew / (2 sin)              pi-1e-3      1.4e+05   (pi-1e-4, pi-1e-6, f32(pi): 1.3e+06 ... 1.4e+06)
    3 quaternion always from the trace pivot               pi-1e-4      inf       (root of a negative number; also pi-1e-6, f32(pi))
    4 the qw < 0 sign rule dropped: norm above pi          pi-1e-3      4.7e+02   (pi+1e-3: 4.8e+02, pi-1e-2: 6.1e+03, 3.0: 8.5e+04,
                                                                                   2pi/3+1e-4: 5.8e+05; pi-1e-6: 0.66 -- not caught)
                                    vector difference      pi-1e-3      2.9e+06   (2pi/3+1e-4 ... pi-1e-2: 3.7e+06 ... 4.8e+06)
    5 sine / cosine one quadrant off for k >= 3            3pi/2        4.9e+05   (2pi-1e-3 ... 20: 2.9e+05 ... 9.2e+05, 100: 4.8e+04)
    6 Rodrigues gradient without the projection            1            1.4e+06   (1e-5: 3.5e+04, 1e-3: 9.4e+03, f32(pi): 9.7e+05, 100: 2.6e+02)
    7 Rodrigues gradient with theta^2 / 2 for 1 - cos      1            5.1e+04   (pi/2: 1.6e+05, 3.0: 6.4e+05, 2pi: 2.4e+06, 100: 3.0e+06;
                                                                                   inside the bound at 1e-4, where the series is the better formula)
    8 Gram-Schmidt without the second normalisation        1 (scaled)   1.0e+09   (inside the bound on exact, unit-length columns)

Yardstick against the caps (1e-5 on matrix entries, 2e-5 on axis-angle vectors up to pi - 1e-3): it stays below them in EVERY band, so
the caps hold in every band.  The angle's own rounding, ulp(theta), shows from 2 pi up -- matrix error 5.2e-7 at 2 pi, 1.1e-6 at 20 rad,
7.05e-6 at 100 rad -- without reaching 1e-5; at 100 rad the cap, not 4 x yardstick (2.8e-5), is what limits the kernel.
Without a cap (``NO_CAP``, with the yardstick's measured worst error):
  * 6-D inputs whose columns are 1e-3 rad apart: 1.9e-4 on matrix entries (input rounding amplified by 1 / sin 1e-3);
  * the Rodrigues gradient, |dR| ~ 1: the hump 2.8e-5 at 1e-5 rad, 2.5e-4 at 1e-4, 2.2e-4 at 3e-4, 1.1e-4 at 1e-3, 4.9e-6 at 1e-2, and
    2.2e-5 at 100 rad, against ~1e-6 elsewhere.  No existing bar applies to single gradient elements.
"""
import numpy as np
import pytest
import torch

import rot_ref as rr
from helpers import _log_measured

NO_CAP = {"rot6d near-parallel": 1.9e-4, "rodrigues vjp 1e-5": 2.8e-5, "rodrigues vjp 1e-4": 2.5e-4, "rodrigues vjp 3e-4": 2.2e-4,
          "rodrigues vjp 1e-3": 1.1e-4, "rodrigues vjp 100": 2.2e-5}       # the yardstick's measured worst error where no cap applies
PIVOT_BANDS = ["2pi/3+1e-4", "3.0", "pi-1e-2", "pi-1e-3", "pi-1e-4", "pi-1e-6", "f32(pi)", "pi+1e-3"]


def _factor(name, band, err, bnd):
    f = err / bnd
    _log_measured(f"planted {name} band {band} factor", f)
    print(f"planted {name}: band {band}: error {err:.3e}, bound {bnd:.3e}, factor {f:.3e}")
    return f


# ------------------------------------------------------------------------------------------------
# conditions on the inputs
# ------------------------------------------------------------------------------------------------
def test_bands_are_the_issue_list_and_inputs_are_float32():
    assert len(rr.BANDS) == 27 and rr.THETA["0"] == 0.0 and rr.THETA["f32(pi)"] == float(np.float32(np.pi))
    for b in rr.BAND_NAMES:
        rv = rr.band_rotvecs(b)
        assert rv.dtype == np.float32 and rv.shape == (rr.N_CONV, 3)
        assert np.array_equal(rv, rr.band_rotvecs(b))                             # fixed seed
        if rr.THETA[b] > 0:
            assert np.abs(np.linalg.norm(rv.astype(np.float64), axis=1) / rr.THETA[b] - 1).max() < 2e-7
    assert not rr.band_rotvecs("0").any()                                         # the exact zero vector


def test_tie_axes_are_present_in_every_band():
    sp = rr.special_axes()
    assert sp.shape == (26, 3) and np.abs(np.linalg.norm(sp, axis=1) - 1).max() < 1e-15
    assert sum(np.count_nonzero(a) == 1 for a in sp) == 6 and sum(np.count_nonzero(a) == 2 for a in sp) == 12
    diag = [a for a in sp if np.count_nonzero(a) == 3]
    assert len(diag) == 8 and all(len(set(np.abs(a))) == 1 for a in diag)
    assert len({tuple(np.sign(a)) for a in sp}) == 26
    for n, stream in ((rr.N_CONV, 0), (rr.N_BODY, 1)):
        for b in rr.BAND_NAMES:
            assert np.array_equal(rr.band_axes(b, n, stream)[:26], sp)
    # the (+-1, +-1, +-1) / sqrt(3) axes give three equal diagonal entries, the (+-1, +-1, 0) / sqrt(2) axes two, in the float32 matrix
    R = rr.rodrigues_truth(rr.band_rotvecs("3.0")).astype(np.float32)
    d = np.stack([R[:, 0, 0], R[:, 1, 1], R[:, 2, 2]], axis=1)
    assert all(d[i, 0] == d[i, 1] == d[i, 2] for i in range(18, 26))
    assert all(len(set(d[i])) == 2 for i in range(6, 18))


def test_every_pivot_of_the_four_case_rule_is_visited():
    """Bands whose rotation angle min(theta mod 2 pi, 2 pi - theta mod 2 pi) is >= 2 pi / 3 + 1e-4 have a negative trace: each of the
    three diagonal pivots gets >= 200 matrices.  (3 pi / 2 and the bands from 2 pi - 1e-3 up are rotations by less than 2 pi / 3.)
    Below 2 pi / 3 - 1e-4 every matrix takes the trace pivot."""
    for b in rr.BAND_NAMES:
        R32 = rr.rodrigues_truth(rr.band_rotvecs(b)).astype(np.float32)
        counts = np.bincount(rr.mat_to_quat_f32(R32)[1], minlength=4)
        eff = rr.effective_angle(rr.THETA[b])
        assert (b in PIVOT_BANDS) == (eff >= 2 * np.pi / 3 + 1e-4 - 1e-12), b
        if b in PIVOT_BANDS:
            assert counts[0] == 0 and counts[1:].min() >= 200, (b, counts)
        else:
            assert eff <= 2 * np.pi / 3 - 1e-4 + 1e-12 and counts[0] == rr.N_CONV, (b, counts)
    # the two bands around 2 pi / 3 straddle the trace = 0 switch
    assert rr.BAND_NAMES.index("2pi/3+1e-4") == rr.BAND_NAMES.index("2pi/3-1e-4") + 1


def test_body_pose_patterns_put_the_band_angle_where_they_say():
    for band in ("1e-4", "f32(pi)", "100"):
        th = rr.THETA[band]
        n = lambda a: np.linalg.norm(a.astype(np.float64), axis=-1)
        root, body = rr.body_poses("root", band)
        assert root.dtype == body.dtype == np.float32 and root.shape == (64, 3) and body.shape == (64, 63)
        assert np.abs(n(root) / th - 1).max() < 2e-7
        for j in (1, 4, 9, 20):
            root, body = rr.body_poses(f"joint{j}", band)
            at = n(body.reshape(64, 21, 3))
            assert np.abs(at[:, j - 1] / th - 1).max() < 2e-7
            assert (np.abs(np.delete(at, j - 1, axis=1) / th - 1) > 1e-3).all()
        root, body = rr.body_poses("all", band)
        assert np.abs(n(body.reshape(64, 21, 3)) / th - 1).max() < 2e-7


# ------------------------------------------------------------------------------------------------
# the yardsticks: finite, and below the existing hard caps
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("band", rr.BAND_NAMES)
def test_yardsticks_are_finite_and_below_the_caps(band):
    rv = rr.band_rotvecs(band)
    T = rr.rodrigues_truth(rv)
    e_rod = rr.max_abs(rr.rodrigues_yard(rv), T)
    assert np.isfinite(e_rod) and e_rod < rr.CAP_MAT and rr.orth_err(rr.rodrigues_yard(rv)) < rr.CAP_MAT
    assert (rr.bound(e_rod, rr.FLOOR_MAT) > rr.CAP_MAT) == (band == "100")       # only there does the cap, not the bound, limit the kernel
    if band == "0":
        assert np.array_equal(rr.rodrigues_yard(rv), np.broadcast_to(np.eye(3, dtype=np.float32), (len(rv), 3, 3)))
        assert np.array_equal(T, np.broadcast_to(np.eye(3), (len(rv), 3, 3)))
    R32 = T.astype(np.float32)
    aa = rr.mat_to_aa_yard(R32)
    e_geo = rr.geodesic(aa, rr.rotation_of(R32))
    assert np.isfinite(e_geo) and e_geo < rr.CAP_AA
    assert np.linalg.norm(aa.astype(np.float64), axis=1).max() <= rr.PI32 + rr.bound(e_geo, rr.FLOOR_AA)      # (three rounded components)
    if rr.THETA[band] <= np.pi - 1e-3:
        assert rr.max_abs(aa, rr.mat_to_aa_truth(R32)) < rr.CAP_AA / 4
    if band == "0":
        assert not aa.any()
    # above pi the vector is the equivalent rotation by 2 pi - theta
    assert abs(np.linalg.norm(aa.astype(np.float64), axis=1) - rr.effective_angle(float(np.linalg.norm(rv[30].astype(np.float64))))).max() < 1e-5
    for six in (rr.sixd_exact(rv), rr.sixd_scaled_sheared(rv)):
        assert rr.max_abs(rr.rot6d_yard(six), T) < rr.CAP_MAT / 4
    par = rr.sixd_near_parallel(rv)
    e_par = rr.max_abs(rr.rot6d_yard(par), rr.rot6d_truth(par))
    assert e_par < 1.5 * NO_CAP["rot6d near-parallel"]
    if 1e-2 <= rr.THETA[band] <= 2 * np.pi - 1e-3:                                # above the cap away from the identity: the cap is not for this input
        assert e_par > rr.CAP_MAT
    dR = rr.cotangent(len(rv), (3, 3))
    g64, g32 = rr.rodrigues_vjp_torch(rv, dR, torch.float64), rr.rodrigues_vjp_torch(rv, dR, torch.float32)
    assert np.isfinite(g64).all() and np.isfinite(g32).all()
    assert rr.max_abs(g32, g64) < 1.5 * NO_CAP.get(f"rodrigues vjp {band}", 1e-5 / 1.5)
    _log_measured(f"yardstick rodrigues {band}", e_rod)
    _log_measured(f"yardstick rodrigues vjp {band}", rr.max_abs(g32, g64))


def test_gradient_hump_of_the_yardstick():
    """torch float32 autograd of smplx's formula: ~3e-4 absolute for |dR| ~ 1 between 1e-5 and 1e-3 rad, ~1e-6 at 0.1 rad and at 1e-7 rad.
    This is why the gradient bounds are per band."""
    e = {}
    for band in ("1e-7", "1e-5", "1e-4", "3e-4", "1e-3", "0.1"):
        rv, dR = rr.band_rotvecs(band), rr.cotangent(rr.N_CONV, (3, 3))
        e[band] = rr.max_abs(rr.rodrigues_vjp_torch(rv, dR, torch.float32), rr.rodrigues_vjp_torch(rv, dR, torch.float64))
    assert e["1e-7"] < 2e-6 and e["0.1"] < 2e-6
    assert 1e-5 < e["1e-5"] < 1e-4 and all(5e-5 < e[b] < 6e-4 for b in ("1e-4", "3e-4", "1e-3"))


@pytest.mark.parametrize("band", rr.BAND_NAMES)
def test_an_honest_float32_statement_meets_the_band_bound(band):
    """The switchable float32 statements below, with every switch in its correct position, are second float32 evaluations of the same
    rules (other operation order, another sine / cosine): they meet the bound the kernels are held to, in every band."""
    rv = rr.band_rotvecs(band)
    T = rr.rodrigues_truth(rv)
    b_rod = rr.bound(rr.max_abs(rr.rodrigues_yard(rv), T), rr.FLOOR_MAT)
    assert rr.max_abs(rr.rodrigues_f32(rv), T) <= b_rod
    assert rr.max_abs(rr.rodrigues_f32(rv, sincos=rr.sincos_quadrants_f32), T) <= b_rod
    dR = rr.cotangent(len(rv), (3, 3))
    g64, g32 = rr.rodrigues_vjp_torch(rv, dR, torch.float64), rr.rodrigues_vjp_torch(rv, dR, torch.float32)
    ratio = rr.max_abs(rr.rodrigues_vjp_f32(rv, dR), g64) / rr.bound(rr.max_abs(g32, g64), rr.grad_floor(g64))
    _log_measured(f"written-out vjp / bound {band}", ratio)
    assert ratio <= 1.0
    six = rr.sixd_scaled_sheared(rv)
    assert rr.max_abs(rr.rot6d_f32(six), T) <= rr.bound(rr.max_abs(rr.rot6d_yard(six), T), rr.FLOOR_MAT)


# ------------------------------------------------------------------------------------------------
# planted errors
# ------------------------------------------------------------------------------------------------
def _aa_setup(band):
    R32 = rr.rodrigues_truth(rr.band_rotvecs(band)).astype(np.float32)
    rot = rr.rotation_of(R32)
    return R32, rot, rr.bound(rr.geodesic(rr.mat_to_aa_yard(R32), rot), rr.FLOOR_AA)


def test_planted_1_rodrigues_without_the_offset():
    rv = rr.band_rotvecs("0")
    T = rr.rodrigues_truth(rv)
    bnd = rr.bound(rr.max_abs(rr.rodrigues_yard(rv), T), rr.FLOOR_MAT)
    assert _factor("1 no offset", "0", rr.max_abs(rr.rodrigues_f32(rv, offset=False), T), bnd) == float("inf")      # 0 / 0
    assert rr.max_abs(rr.rodrigues_f32(rv), T) == 0.0


@pytest.mark.parametrize("band,least", [("pi-1e-3", 20), ("pi-1e-4", 100), ("pi-1e-6", 1e5), ("f32(pi)", 1e5)])
def test_planted_2_log_map_through_acos(band, least):
    R32, rot, bnd = _aa_setup(band)
    assert _factor("2 acos log map", band, rr.geodesic(rr.mat_to_aa_acos_f32(R32), rot), bnd) > least


@pytest.mark.parametrize("band,least", [("pi-1e-4", 30), ("pi-1e-6", 1e3), ("f32(pi)", 1e5)])
def test_planted_3_quaternion_always_from_the_trace(band, least):
    R32, rot, bnd = _aa_setup(band)
    got = rr.quat_to_aa_f32(rr.mat_to_quat_f32(R32, pivot="trace")[0])
    assert _factor("3 trace pivot only", band, rr.geodesic(got, rot), bnd) > least


@pytest.mark.parametrize("band", ["2pi/3+1e-4", "3.0", "pi-1e-2", "pi-1e-3", "pi+1e-3"])
def test_planted_4_sign_rule_dropped(band):
    """Without the rule a negative qw gives an angle in (pi, 2 pi): the same rotation (the geodesic measure does not see it), a vector
    longer than pi (the norm check does), and far from the truth (the vector difference does, where it is taken)."""
    R32, rot, bnd = _aa_setup(band)
    q = rr.mat_to_quat_f32(R32)[0]
    assert (q[:, 0] < 0).sum() > 100
    got = rr.quat_to_aa_f32(q, sign_rule=False).astype(np.float64)
    assert rr.geodesic(got, rot) <= bnd
    over = np.linalg.norm(got, axis=1).max() - rr.PI32
    assert _factor("4 no sign rule (norm - pi)", band, over, bnd) > 400
    if rr.THETA[band] <= np.pi - 1e-3:
        tr = rr.mat_to_aa_truth(R32)
        bv = rr.bound(rr.max_abs(rr.mat_to_aa_yard(R32), tr), rr.FLOOR_AA)
        assert _factor("4 no sign rule (vector)", band, rr.max_abs(got, tr), bv) > 1e5


@pytest.mark.parametrize("band", ["3pi/2", "2pi-1e-3", "2pi", "7", "20", "100"])
def test_planted_5_quadrant_off_by_one(band):
    rv = rr.band_rotvecs(band)
    T = rr.rodrigues_truth(rv)
    bnd = rr.bound(rr.max_abs(rr.rodrigues_yard(rv), T), rr.FLOOR_MAT)
    bad = rr.rodrigues_f32(rv, sincos=lambda x: rr.sincos_quadrants_f32(x, off_by_one_from=3))
    assert _factor("5 quadrant", band, rr.max_abs(bad, T), bnd) > 1e4
    # ... and not below k = 3: the bands the existing tests visit do not see it
    lo = rr.band_rotvecs("pi+1e-3")
    assert np.array_equal(rr.rodrigues_f32(lo, sincos=lambda x: rr.sincos_quadrants_f32(x, off_by_one_from=3)),
                          rr.rodrigues_f32(lo, sincos=rr.sincos_quadrants_f32))


def _vjp_setup(band):
    rv, dR = rr.band_rotvecs(band), rr.cotangent(rr.N_CONV, (3, 3))
    g64 = rr.rodrigues_vjp_torch(rv, dR, torch.float64)
    return rv, dR, g64, rr.bound(rr.max_abs(rr.rodrigues_vjp_torch(rv, dR, torch.float32), g64), rr.grad_floor(g64))


@pytest.mark.parametrize("band", ["1e-5", "1e-3", "1", "f32(pi)", "100"])
def test_planted_6_gradient_without_the_projection(band):
    rv, dR, g64, bnd = _vjp_setup(band)
    assert _factor("6 no projection", band, rr.max_abs(rr.rodrigues_vjp_f32(rv, dR, project=False), g64), bnd) > 100


@pytest.mark.parametrize("band", ["1", "pi/2", "3.0", "2pi", "100"])
def test_planted_7_gradient_with_the_series_for_one_minus_cos(band):
    rv, dR, g64, bnd = _vjp_setup(band)
    assert _factor("7 series 1 - cos", band, rr.max_abs(rr.rodrigues_vjp_f32(rv, dR, series_c1=True), g64), bnd) > 1e4
    # in the hump bands the series is the better formula and stays inside the bound: only bands >= 1 can catch this
    rv, dR, g64, bnd = _vjp_setup("1e-4")
    assert rr.max_abs(rr.rodrigues_vjp_f32(rv, dR, series_c1=True), g64) <= bnd


def test_planted_8_gram_schmidt_without_the_second_normalisation():
    rv = rr.band_rotvecs("1")
    T = rr.rodrigues_truth(rv)
    six = rr.sixd_scaled_sheared(rv)
    bnd = rr.bound(rr.max_abs(rr.rot6d_yard(six), T), rr.FLOOR_MAT)
    assert _factor("8 one normalisation", "1 (scaled)", rr.max_abs(rr.rot6d_f32(six, second_normalisation=False), T), bnd) > 1e6
    # on exact columns the second column is already of unit length: the unscaled input cannot catch it
    ex = rr.sixd_exact(rv)
    assert rr.max_abs(rr.rot6d_f32(ex, second_normalisation=False), T) <= rr.bound(rr.max_abs(rr.rot6d_yard(ex), T), rr.FLOOR_MAT)
