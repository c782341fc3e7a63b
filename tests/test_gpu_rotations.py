"""The rotation kernels, the body-model kernels that call them and the two plain-torch differentiable helpers, per ANGLE BAND against
float64 truths (tests/rot_ref.py: 27 bands from the exact zero vector over 1e-8 ... 1e-3, 2 pi / 3 -+ 1e-4, pi - 1e-6, float32(pi),
2 pi up to 100 rad; 1024 axes per band with the tie axes, 64 bodies per band).  In every band

    worst error of the GPU code  <=  min(4 x worst error of the float32 CPU yardstick on the same samples + floor, existing hard cap)

(the caps: 1e-5 on matrix entries and joints in every band -- not for 6-D inputs with near-parallel columns, where the yardstick itself
is at 1.9e-4 --, 2e-5 on axis-angle vectors below pi, 2e-5 as rotations below 3.1 rad for the 6-D -> axis-angle helper).  Gradients
are compared element by element, as the maximum over samples, joints and components, never as one norm.  tests/test_rot_ref_cpu.py
shows on the CPU that eight planted errors break these bounds.

The 6-D -> axis-angle helper as rotation matrices (the measure of tests/test_host_cpu.py, which accepts 2e-3 above 3.1 rad): at most
6.4e-7 in every band -- 4.9e-7 at pi - 1e-2 ... pi - 1e-4, 4.7e-7 at pi - 1e-6, 4.5e-7 at float32(pi).

MEASURED on an MI355X: error / limit per test and band -- the worst of the test's measures, '-' where the band is not run; tests whose
two kernel paths give the same figures share a row.  Every single ratio is passed through helpers._log_measured (DPOSER_LOG_ERR=<file>).
The largest: 0.93 (joint gradient) and 0.73 (joints) with all 21 body joints at 7 rad; there the reduced argument of the kernels'
sine / cosine, 7 - 4 pi / 2 = 0.717, lies near the edge of its polynomials' range [-pi/4, pi/4] -- the likely reason, not established.
Column heads: +1e-3 = pi/2 + 1e-3, 2pi/3- and 2pi/3+ = 2 pi / 3 -+ 1e-4, pi-e-2 = pi - 1e-2 and so on, f32pi = float32(pi).

                                                       0    1e-8    1e-7    1e-5    1e-4    3e-4    1e-3    1e-2     0.1       1    pi/2   +1e-3  2pi/3-  2pi/3+
                                                     3.0  pi-e-2  pi-e-3  pi-e-4  pi-e-6   f32pi  pi+e-3   3pi/2 2pi-e-3     2pi       7      20     100
    rodrigues                                       0.00    0.00    0.00    0.00    0.06    0.18    0.19    0.18    0.19    0.25    0.52    0.27    0.25    0.38
                                                    0.40    0.35    0.26    0.21    0.32    0.26    0.25    0.30    0.25    0.22    0.37    0.40    0.33
    axis_angle_to_rot6d                             0.00    0.00    0.00    0.00    0.04    0.14    0.16    0.14    0.15    0.25    0.58    0.31    0.25    0.38
                                                    0.42    0.32    0.25    0.28    0.28    0.26    0.25    0.30    0.25    0.22    0.37    0.40    0.33
    rot6d_to_mat3x3[exact]                          0.00    0.00    0.00    0.00    0.06    0.23    0.21    0.22    0.23    0.23    0.23    0.23    0.23    0.23
                                                    0.23    0.23    0.23    0.23    0.23    0.23    0.23    0.23    0.21    0.00    0.23    0.23    0.23
    rot6d_to_mat3x3[scaled+sheared]                 0.00    0.06    0.12    0.12    0.13    0.23    0.24    0.23    0.23    0.23    0.23    0.24    0.23    0.23
                                                    0.23    0.23    0.23    0.23    0.23    0.23    0.23    0.23    0.24    0.12    0.23    0.23    0.23
    rot6d_to_mat3x3[near-parallel]                  0.00    0.06    0.19    0.25    0.25    0.25    0.25    0.25    0.25    0.25    0.25    0.25    0.25    0.25
                                                    0.25    0.25    0.25    0.25    0.25    0.25    0.25    0.25    0.25    0.22    0.25    0.25    0.25
    rotmat_to_axis_angle[exact matrices]            0.00    0.00    0.00    0.00    0.00    0.00    0.00    0.01    0.05    0.19    0.27    0.15    0.35    0.22
                                                    0.21    0.21    0.22    0.22    0.22    0.23    0.22    0.27    0.00    0.00    0.16    0.17    0.24
    rotmat_to_axis_angle[kernel's matrices]         0.00    0.00    0.00    0.00    0.00    0.00    0.00    0.01    0.06    0.28    0.39    0.23    0.23    0.22
                                                    0.25    0.30    0.22    0.22    0.22    0.23    0.22    0.25    0.00    0.00    0.16    0.36    0.15
    rot6d_to_axis_angle[exact]                      0.00    0.00    0.00    0.00    0.00    0.00    0.00    0.01    0.05    0.19    0.25    0.17    0.30    0.22
                                                    0.21    0.22    0.22    0.22    0.22    0.22    0.23    0.31    0.00    0.00    0.17    0.17    0.22
    rot6d_to_axis_angle[scaled+sheared]             0.00    0.02    0.05    0.05    0.05    0.13    0.14    0.15    0.14    0.27    0.22    0.19    0.28    0.20
                                                    0.21    0.22    0.23    0.22    0.22    0.22    0.22    0.31    0.13    0.05    0.20    0.20    0.22
    rot6d_to_axis_angle[near-parallel]              0.00    0.02    0.11    0.25    0.25    0.25    0.25    0.25    0.25    0.25    0.25    0.25    0.25    0.25
                                                    0.25    0.25    0.25    0.25    0.25    0.25    0.25    0.25    0.25    0.17    0.25    0.25    0.25
    row counts[1]                                      -       -       -       -       -       -       -       -       -       -       -       -       -       -
                                                    0.16       -       -       -       -       -       -       -       -       -       -       -       -
    row counts[255] = [256], [257]                     -       -       -       -       -       -       -       -       -       -       -       -       -       -
                                                    0.37       -       -       -       -       -       -       -       -       -       -       -       -
    fk_joints[root], both paths                     0.19    0.19    0.22    0.18    0.17    0.26    0.21    0.19    0.21    0.17    0.32    0.21    0.21    0.29
                                                    0.35    0.23    0.18    0.20    0.41    0.20    0.26    0.35    0.32    0.15    0.40    0.46    0.16
    fk_joints[joint1], both paths                   0.28    0.28    0.28    0.28    0.28    0.28    0.28    0.28    0.28    0.28    0.28    0.28    0.28    0.28
                                                    0.28    0.28    0.28    0.28    0.28    0.23    0.28    0.28    0.28    0.28    0.28    0.53    0.16
    fk_joints[joint4], both paths                   0.24    0.24    0.24    0.24    0.24    0.24    0.24    0.24    0.24    0.24    0.24    0.24    0.24    0.24
                                                    0.23    0.26    0.20    0.26    0.27    0.19    0.23    0.24    0.27    0.20    0.39    0.32    0.15
    fk_joints[joint9], both paths                   0.27    0.21    0.17    0.23    0.20    0.26    0.19    0.24    0.20    0.23    0.30    0.26    0.20    0.24
                                                    0.34    0.31    0.17    0.28    0.40    0.19    0.31    0.25    0.43    0.23    0.52    0.53    0.13
    fk_joints[joint20], both paths                  0.25    0.25    0.25    0.25    0.25    0.25    0.25    0.25    0.25    0.25    0.25    0.25    0.25    0.25
                                                    0.25    0.25    0.25    0.25    0.25    0.25    0.25    0.25    0.25    0.25    0.25    0.25    0.25
    fk_joints[all], both paths                      0.19    0.17    0.22    0.16    0.27    0.24    0.24    0.21    0.23    0.21    0.36    0.33    0.20    0.33
                                                    0.50    0.32    0.19    0.39    0.54    0.21    0.28    0.28    0.41    0.21    0.73    0.33    0.20
    joint_gradient[root], both paths                0.24    0.21    0.29    0.24    0.25    0.25    0.25    0.28    0.18    0.26    0.29    0.25    0.22    0.23
                                                    0.24    0.18    0.13    0.19    0.38    0.29    0.28    0.33    0.24    0.30    0.44    0.35    0.17
    joint_gradient[joint1], both paths              0.24    0.24    0.24    0.23    0.25    0.25    0.25    0.24    0.24    0.23    0.24    0.24    0.24    0.24
                                                    0.24    0.24    0.24    0.24    0.24    0.24    0.25    0.24    0.24    0.24    0.23    0.25    0.22
    joint_gradient[joint4], both paths              0.25    0.25    0.25    0.25    0.25    0.25    0.25    0.22    0.27    0.23    0.22    0.25    0.25    0.25
                                                    0.26    0.25    0.24    0.25    0.28    0.25    0.28    0.25    0.25    0.25    0.29    0.36    0.25
    joint_gradient[joint9], both paths              0.40    0.41    0.47    0.25    0.25    0.25    0.25    0.19    0.43    0.30    0.24    0.24    0.27    0.29
                                                    0.33    0.36    0.23    0.20    0.21    0.28    0.28    0.25    0.35    0.30    0.28    0.28    0.20
    joint_gradient[joint20], both paths             0.27    0.27    0.27    0.27    0.27    0.27    0.27    0.27    0.27    0.27    0.27    0.27    0.27    0.27
                                                    0.27    0.27    0.27    0.27    0.27    0.27    0.27    0.27    0.27    0.27    0.27    0.27    0.27
    joint_gradient[all], both paths                 0.26    0.23    0.36    0.24    0.25    0.25    0.25    0.22    0.27    0.25    0.23    0.26    0.29    0.30
                                                    0.58    0.32    0.17    0.30    0.25    0.14    0.19    0.31    0.31    0.18    0.93    0.41    0.20
    full_gradient[root-default]                     0.27    0.27    0.27    0.24    0.25    0.25    0.25    0.24    0.27    0.28    0.24    0.23    0.21    0.17
                                                    0.38    0.26    0.19    0.44    0.38    0.26    0.35    0.28    0.35    0.16    0.56    0.38    0.19
    full_gradient[root-streaming]                   0.25    0.29    0.27    0.24    0.25    0.25    0.25    0.26    0.26    0.26    0.27    0.28    0.22    0.20
                                                    0.37    0.28    0.20    0.56    0.38    0.26    0.33    0.24    0.32    0.21    0.41    0.32    0.19
    full_gradient[joint1-default]                   0.29    0.29    0.30    0.24    0.25    0.25    0.25    0.23    0.19    0.19    0.29    0.23    0.22    0.17
                                                    0.17    0.24    0.22    0.16    0.22    0.26    0.22    0.20    0.21    0.18    0.22    0.20    0.15
    full_gradient[joint1-streaming]                 0.25    0.25    0.24    0.24    0.25    0.25    0.25    0.23    0.19    0.24    0.25    0.19    0.20    0.30
                                                    0.29    0.25    0.20    0.18    0.22    0.25    0.32    0.26    0.29    0.34    0.34    0.25    0.15
    full_gradient[joint4-default]                   0.22    0.22    0.22    0.24    0.25    0.25    0.25    0.22    0.20    0.19    0.23    0.15    0.24    0.18
                                                    0.22    0.23    0.25    0.23    0.26    0.20    0.22    0.15    0.22    0.19    0.33    0.26    0.25
    full_gradient[joint4-streaming]                 0.22    0.22    0.24    0.24    0.25    0.25    0.25    0.21    0.35    0.21    0.22    0.15    0.24    0.25
                                                    0.26    0.19    0.25    0.20    0.26    0.18    0.24    0.19    0.20    0.20    0.32    0.21    0.24
    full_gradient[joint9-default]                   0.27    0.27    0.17    0.25    0.25    0.25    0.25    0.24    0.16    0.22    0.33    0.20    0.16    0.26
                                                    0.45    0.19    0.17    0.31    0.35    0.22    0.48    0.29    0.41    0.25    0.28    0.35    0.24
    full_gradient[joint9-streaming]                 0.26    0.25    0.21    0.25    0.25    0.25    0.25    0.25    0.17    0.22    0.30    0.23    0.22    0.26
                                                    0.53    0.14    0.28    0.33    0.36    0.23    0.51    0.25    0.39    0.28    0.31    0.35    0.24
    full_gradient[joint20-default]                  0.24    0.24    0.22    0.25    0.25    0.25    0.25    0.22    0.20    0.28    0.24    0.26    0.24    0.29
                                                    0.45    0.25    0.22    0.23    0.36    0.24    0.35    0.26    0.22    0.32    0.40    0.28    0.25
    full_gradient[joint20-streaming]                0.26    0.26    0.26    0.25    0.25    0.25    0.25    0.21    0.18    0.23    0.22    0.28    0.29    0.22
                                                    0.40    0.24    0.20    0.28    0.25    0.34    0.40    0.24    0.22    0.24    0.36    0.29    0.25
    full_gradient[all-default]                      0.30    0.39    0.26    0.25    0.25    0.25    0.25    0.24    0.25    0.26    0.26    0.32    0.35    0.24
                                                    0.34    0.63    0.23    0.39    0.40    0.15    0.22    0.31    0.50    0.29    0.81    0.46    0.18
    full_gradient[all-streaming]                    0.21    0.39    0.18    0.25    0.25    0.25    0.25    0.24    0.18    0.23    0.29    0.33    0.34    0.27
                                                    0.39    0.53    0.16    0.39    0.42    0.22    0.22    0.29    0.39    0.24    0.82    0.52    0.18
    root gradient, default blend                    0.34    0.39    0.49    0.25    0.25    0.25    0.25    0.24    0.44    0.34    0.22    0.35    0.25    0.26
                                                    0.26    0.44    0.35    0.28    0.36    0.48    0.29    0.35    0.25    0.28    0.32    0.35    0.34
    axis_angle_to_rot6d helper                      0.19    0.13    0.20    0.25    0.25    0.25    0.25    0.24    0.21    0.26    0.25    0.23    0.24    0.22
                                                    0.22    0.23    0.24    0.26    0.25    0.24    0.24    0.20    0.24    0.26    0.24    0.27    0.70
    rot6d_to_axis_angle helper                      0.00    0.08    0.17    0.18    0.20    0.25    0.21    0.22    0.25    0.25    0.22    0.32    0.35    0.21
                                                    0.25    0.30    0.24    0.24    0.31    0.33       -       -       -       -       -       -       -
"""
import numpy as np
import pytest
import torch
from scipy.spatial.transform import Rotation

import rot_ref as rr
from gpu_common import DEV, t2n
from helpers import _log_measured

pytestmark = pytest.mark.gpu


class _Ledger:
    """Collects (band, measure, error, limit) of one test, logs every ratio and fails at the end with all offenders."""

    def __init__(self):
        self.rows = []

    def add(self, band, what, err, yard, floor, cap=None):
        lim = rr.bound(yard, floor)
        if cap is not None:
            lim = min(lim, cap)
        ratio = float(err) / lim
        _log_measured(f"band {band} | {what} | err {err:.3e} yard {yard:.3e} limit {lim:.3e} | ratio", ratio)
        self.rows.append((band, what, float(err), float(yard), lim, ratio))

    def check(self):
        worst = max(self.rows, key=lambda r: r[5])
        print(f"worst ratio {worst[5]:.2f} in band {worst[0]} ({worst[1]}: err {worst[2]:.3e}, yardstick {worst[3]:.3e}, limit {worst[4]:.3e})")
        bad = [r for r in self.rows if not r[5] <= 1.0]
        assert not bad, bad


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a), device=DEV)


# ------------------------------------------------------------------------------------------------
# conversions
# ------------------------------------------------------------------------------------------------
def test_rodrigues_by_band():
    from dposer_amd.utils.transforms import axis_angle_to_mat3x3, batch_rodrigues
    led = _Ledger()
    for band in rr.BAND_NAMES:
        rv = rr.band_rotvecs(band)
        T, Y = rr.rodrigues_truth(rv), rr.rodrigues_yard(rv)
        out = batch_rodrigues(_dev(rv))
        assert torch.equal(out, axis_angle_to_mat3x3(_dev(rv)))
        out = t2n(out)
        led.add(band, "entries", rr.max_abs(out, T), rr.max_abs(Y, T), rr.FLOOR_MAT, rr.CAP_MAT)
        led.add(band, "R R^T - I", rr.orth_err(out), rr.orth_err(Y), rr.FLOOR_MAT, rr.CAP_MAT)
        if band == "0":
            assert np.array_equal(out, np.broadcast_to(np.eye(3, dtype=np.float32), out.shape))          # bit for bit
    led.check()


def test_axis_angle_to_rot6d_by_band():
    from dposer_amd.utils.transforms import axis_angle_to_rot6d
    led = _Ledger()
    for band in rr.BAND_NAMES:
        rv = rr.band_rotvecs(band)
        T, Y = rr.rodrigues_truth(rv)[:, :, :2].reshape(-1, 6), rr.rodrigues_yard(rv)[:, :, :2].reshape(-1, 6)
        out = t2n(axis_angle_to_rot6d(_dev(rv)))
        assert out.shape == (rr.N_CONV, 6)
        led.add(band, "two columns, row-major", rr.max_abs(out, T), rr.max_abs(Y, T), rr.FLOOR_MAT, rr.CAP_MAT)
    led.check()


_SIXD = {"exact": rr.sixd_exact, "scaled+sheared": rr.sixd_scaled_sheared, "near-parallel": rr.sixd_near_parallel}


@pytest.mark.parametrize("kind", list(_SIXD))
def test_rot6d_to_mat3x3_by_band(kind):
    """'near-parallel': the yardstick's own error is ~1e-4 there (rounding of the inputs' difference, amplified by 1 / sin 1e-3): no cap."""
    from dposer_amd.utils.transforms import rot6d_to_mat3x3
    led = _Ledger()
    cap = None if kind == "near-parallel" else rr.CAP_MAT
    for band in rr.BAND_NAMES:
        six = _SIXD[kind](rr.band_rotvecs(band))
        T, Y = rr.rot6d_truth(six), rr.rot6d_yard(six)
        out = t2n(rot6d_to_mat3x3(_dev(six)))
        led.add(band, "entries", rr.max_abs(out, T), rr.max_abs(Y, T), rr.FLOOR_MAT, cap)
        led.add(band, "R R^T - I", rr.orth_err(out), rr.orth_err(Y), rr.FLOOR_MAT, cap)
        assert np.linalg.det(out.astype(np.float64)).min() > 0.99
    led.check()


def _axis_angle_measures(led, band, theta_in, out, yard, rot, vec_truth):
    """geodesic angle in every band; plain vector difference up to pi - 1e-3; norm <= float32(pi) + bound; the vector's length is the
    rotation angle in [0, pi] -- 2 pi - theta for an input angle theta in (pi, 2 pi)."""
    g_y = rr.geodesic(yard, rot)
    led.add(band, "geodesic", rr.geodesic(out, rot), g_y, rr.FLOOR_AA, rr.CAP_AA)
    if rr.THETA[band] <= np.pi - 1e-3:
        led.add(band, "vector", rr.max_abs(out, vec_truth), rr.max_abs(yard, vec_truth), rr.FLOOR_AA, rr.CAP_AA)
    norm = np.linalg.norm(out.astype(np.float64), axis=1)
    led.add(band, "norm - float32(pi)", max(0.0, float(norm.max()) - rr.PI32), g_y, rr.FLOOR_AA)
    eff = np.array([rr.effective_angle(t) for t in theta_in])
    led.add(band, "norm - rotation angle", rr.max_abs(norm, eff),
            rr.max_abs(np.linalg.norm(yard.astype(np.float64), axis=1), eff), rr.FLOOR_AA)


@pytest.mark.parametrize("source", ["exact matrices", "the Rodrigues kernel's matrices"])
def test_rotmat_to_axis_angle_by_band(source):
    from dposer_amd.utils.transforms import batch_rodrigues, rotmat_to_axis_angle
    led = _Ledger()
    for band in rr.BAND_NAMES:
        rv = rr.band_rotvecs(band)
        R32 = rr.rodrigues_truth(rv).astype(np.float32) if source == "exact matrices" else t2n(batch_rodrigues(_dev(rv)))
        rot = rr.rotation_of(R32)
        yard = rr.mat_to_aa_yard(R32)
        out_d = rotmat_to_axis_angle(_dev(R32))
        out = t2n(out_d)
        if source == "exact matrices" and np.pi < rr.THETA[band] < 2 * np.pi:                        # the truth itself: the equivalent rotation by 2 pi - theta
            assert np.abs(rot.magnitude() - (2 * np.pi - np.linalg.norm(rv.astype(np.float64), axis=1))).max() < 1e-6
        _axis_angle_measures(led, band, rot.magnitude(), out, yard, rot, rot.as_rotvec())
        if band == "0":
            assert not out.any()                                       # identity -> the zero vector, bit for bit
        if source != "exact matrices":                                 # matrix -> vector -> matrix, compared as rotations
            back = t2n(batch_rodrigues(out_d))
            led.add(band, "round trip", rr.geodesic_mats(back, rot), rr.geodesic_mats(rr.rodrigues_yard(yard), rot), rr.FLOOR_AA, rr.CAP_AA)
    led.check()


@pytest.mark.parametrize("kind", list(_SIXD))
def test_rot6d_to_axis_angle_by_band(kind):
    from dposer_amd.utils.transforms import rot6d_to_axis_angle
    led = _Ledger()
    for band in rr.BAND_NAMES:
        rv = rr.band_rotvecs(band)
        six = _SIXD[kind](rv)
        rot = Rotation.from_matrix(rr.rot6d_truth(six))
        yard = rr.mat_to_aa_yard(rr.rot6d_yard(six))
        out = t2n(rot6d_to_axis_angle(_dev(six)))
        if kind == "near-parallel":                                    # (the amplified rounding is in the yardstick; no cap)
            led.add(band, "geodesic", rr.geodesic(out, rot), rr.geodesic(yard, rot), rr.FLOOR_AA)
        else:
            _axis_angle_measures(led, band, rot.magnitude(), out, yard, rot, rot.as_rotvec())
        if band == "0" and kind != "near-parallel":
            assert not out.any()                                       # 6-D identity (also scaled) -> the zero vector, bit for bit
    led.check()


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_row_counts_around_one_block(n):
    """One band, every entry point: n rows give the bits of the first n rows of the 1024-row call, and meet the band bound."""
    from dposer_amd.utils import transforms as tf
    band = "3.0"
    rv = rr.band_rotvecs(band)
    six = rr.sixd_scaled_sheared(rv)
    R32 = rr.rodrigues_truth(rv).astype(np.float32)
    led = _Ledger()
    for name, fn, x in (("batch_rodrigues", tf.batch_rodrigues, rv), ("axis_angle_to_rot6d", tf.axis_angle_to_rot6d, rv),
                        ("rot6d_to_mat3x3", tf.rot6d_to_mat3x3, six), ("rotmat_to_axis_angle", tf.rotmat_to_axis_angle, R32),
                        ("rot6d_to_axis_angle", tf.rot6d_to_axis_angle, six)):
        full, part = fn(_dev(x)), fn(_dev(x[:n]))
        assert part.shape[0] == n and torch.equal(part, full[:n]), name
    # the yardstick's worst error is taken over the band's 1024 samples (over 1 or 255 rows it is not a worst case; the first row, axis
    # e_x, has a yardstick error of 1.5e-8)
    T = rr.rodrigues_truth(rv)
    led.add(band, "rodrigues", rr.max_abs(t2n(tf.batch_rodrigues(_dev(rv[:n]))), T[:n]), rr.max_abs(rr.rodrigues_yard(rv), T), rr.FLOOR_MAT, rr.CAP_MAT)
    led.add(band, "rot6d", rr.max_abs(t2n(tf.rot6d_to_mat3x3(_dev(six[:n]))), T[:n]), rr.max_abs(rr.rot6d_yard(six), T), rr.FLOOR_MAT, rr.CAP_MAT)
    led.add(band, "rotmat_to_axis_angle", rr.geodesic(t2n(tf.rotmat_to_axis_angle(_dev(R32[:n]))), rr.rotation_of(R32[:n])),
            rr.geodesic(rr.mat_to_aa_yard(R32), rr.rotation_of(R32)), rr.FLOOR_AA, rr.CAP_AA)
    led.check()


# ------------------------------------------------------------------------------------------------
# the body model: joints and gradients, three pose patterns, the small-batch and the general kernels
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bm():
    from dposer_amd.body_model.body_model import BodyModel
    return BodyModel(rr.body_asset(), num_betas=10, num_expressions=0, model_type="smplx").to(DEV)


def _floor_of(a):
    return rr.FLOOR_MAT * float(np.abs(a).max())


@pytest.mark.parametrize("path", ["small-batch kernels", "general kernels"])
@pytest.mark.parametrize("pattern", rr.PATTERNS)
def test_fk_joints_by_band(bm, tuning_env, pattern, path):
    if path == "general kernels":
        tuning_env(DPOSER_FK_SMALL_MAX="0")
    ref = rr.body_reference(pattern)
    led = _Ledger()
    with torch.no_grad():
        for band in rr.BAND_NAMES:
            root, body = rr.body_poses(pattern, band)
            j = t2n(bm.fk_joints(_dev(body), root_orient=_dev(root), n_joints=22))
            s = rr.band_rows(band)
            T, Y = ref["joints_truth"][s], ref["joints_yard"][s]
            led.add(band, "22 joints", rr.max_abs(j, T), rr.max_abs(Y, T), _floor_of(T), rr.CAP_MAT)
    led.check()


def _gradient_by_band(bm, pattern, loss, led, root_only=False):
    ref = rr.body_reference(pattern)
    wj, wv = rr.body_weights()
    wj_d, wv_d = _dev(wj), _dev(wv)
    for band in rr.BAND_NAMES:
        root, body = rr.body_poses(pattern, band)
        r, p = _dev(root).requires_grad_(True), _dev(body).requires_grad_(True)
        if loss == "joints":
            val = (bm.fk_joints(p, root_orient=r, n_joints=22) * wj_d[:, :22]).sum()
        else:
            o = bm(pose_body=p, root_orient=r)
            val = (o.Jtr * wj_d).sum() + (o.v * wv_d).sum()
        gr, gp = torch.autograd.grad(val, [r, p])
        g = np.concatenate([t2n(gr), t2n(gp)], axis=1)
        s = rr.band_rows(band)
        T, Y = ref[f"grad_{loss}_truth"][s], ref[f"grad_{loss}_yard"][s]
        cols = slice(0, 3) if root_only else slice(0, 66)
        led.add(band, f"d {loss} loss / d {'root_orient' if root_only else '(root_orient, pose_body)'}", rr.max_abs(g[:, cols], T[:, cols]),
                rr.max_abs(Y[:, cols], T[:, cols]), _floor_of(T[:, cols]))


@pytest.mark.parametrize("path", ["k_fk_bwd_small", "k_fk_bwd"])
@pytest.mark.parametrize("pattern", rr.PATTERNS)
def test_joint_gradient_by_band(bm, tuning_env, pattern, path):
    """Loss on the 22 body joints only (a differentiable BodyModel.fk_joints): the chain backward and rodrigues_bwd."""
    if path == "k_fk_bwd":
        tuning_env(DPOSER_FK_SMALL_MAX="0")
    led = _Ledger()
    _gradient_by_band(bm, pattern, "joints", led)
    led.check()


@pytest.mark.parametrize("backward", ["default backward", "streaming backward"])
@pytest.mark.parametrize("pattern", rr.PATTERNS)
def test_full_gradient_by_band(bm, tuning_env, pattern, backward):
    """All 127 joints plus the vertices with the exact-fp32 pose blend (the default blend runs on bf16 x 3 planes, has its own test and
    would hide what this one is about)."""
    env = dict(DPOSER_LBS_BLEND="fp32")
    if backward == "streaming backward":
        env["DPOSER_LBS_JOINT_STREAM_MIN"] = "1"
    tuning_env(**env)
    led = _Ledger()
    _gradient_by_band(bm, pattern, "full", led)
    led.check()


def test_root_orientation_under_the_default_blend_by_band(bm):
    """The root joint is outside the pose feature, so the default (bf16 x 3) blend does not see the band's angle: the gradient w.r.t. the
    root orientation meets the band bound, and a root orientation acts rigidly, x' = J_root + R (x - J_root), at the existing 1e-5 bar
    in the bands up to 2 pi."""
    led = _Ledger()
    _gradient_by_band(bm, "root", "full", led, root_only=True)
    led.check()
    asset = rr.body_asset()
    Jr = (asset["J_regressor"].astype(np.float64) @ asset["v_template"].astype(np.float64))[0]
    worst = 0.0
    with torch.no_grad():
        for band in rr.BAND_NAMES[:rr.BAND_NAMES.index("2pi") + 1]:
            root, body = rr.body_poses("root", band)
            o0, o1 = bm(pose_body=_dev(body)), bm(pose_body=_dev(body), root_orient=_dev(root))
            R = Rotation.from_rotvec(root.astype(np.float64)).as_matrix()
            for a0, a1 in ((t2n(o0.v), t2n(o1.v)), (t2n(o0.Jtr), t2n(o1.Jtr))):
                want = np.einsum("bij,bnj->bni", R, a0.astype(np.float64) - Jr) + Jr
                err = rr.max_abs(a1, want)
                _log_measured(f"band {band} | rigid action of the root orientation", err)
                worst = max(worst, err)
                assert err < 1e-5, (band, err)
    print(f"rigid action: worst {worst:.3e}")


# ------------------------------------------------------------------------------------------------
# the two plain-torch differentiable helpers, float32 on the GPU (yardstick: the same torch code in float32 on the CPU)
# ------------------------------------------------------------------------------------------------
def _vjp(fn, x, cot):
    x = x.clone().requires_grad_(True)
    out = fn(x)
    (g,) = torch.autograd.grad((out * cot).sum(), [x])
    return out.detach(), g


def test_axis_angle_to_rot6d_autograd_helper_by_band():
    from oracle import fk_torch
    from dposer_amd.tasks.motion_denoising import _axis_angle_to_rot6d_autograd as helper
    ref_fn = lambda x: fk_torch.batch_rodrigues(x)[:, :, :2].reshape(-1, 6)
    cot = rr.cotangent(rr.N_CONV, (6,))
    led = _Ledger()
    for band in rr.BAND_NAMES:
        rv = rr.band_rotvecs(band)
        v64, g64 = _vjp(ref_fn, torch.tensor(rv, dtype=torch.float64), torch.tensor(cot, dtype=torch.float64))
        v32, g32 = _vjp(ref_fn, torch.tensor(rv), torch.tensor(cot))
        v, g = _vjp(helper, _dev(rv), _dev(cot))
        assert v.dtype == torch.float32 and g.dtype == torch.float32
        led.add(band, "value", rr.max_abs(t2n(v), v64.numpy()), rr.max_abs(v32.numpy(), v64.numpy()), rr.FLOOR_MAT, rr.CAP_MAT)
        led.add(band, "gradient", rr.max_abs(t2n(g), g64.numpy()), rr.max_abs(g32.numpy(), g64.numpy()), _floor_of(g64.numpy()))
    led.check()


def test_rot6d_to_axis_angle_autograd_helper_by_band():
    """Bands up to float32(pi); the helper is piecewise (angle < 1e-4: series; cos < -0.99, i.e. above 3.0001 rad: the diagonal route)
    and the bands straddle both switches (1e-5 | 1e-4 ... and 3.0 | pi - 1e-2).  Value: geodesic angle to the truth, and -- the bar of
    tests/test_host_cpu.py -- 2e-5 as rotation matrices below 3.1 rad.  Gradient: the vector-Jacobian product of a fixed cotangent
    against float64 autograd of the same function."""
    from dposer_amd.algorithms.advanced.losses import _rot6d_to_axis_angle_autograd as helper
    bands = rr.BAND_NAMES[:rr.BAND_NAMES.index("f32(pi)") + 1]
    assert rr.THETA["1e-5"] < 1e-4 <= rr.THETA["1e-4"] and np.cos(rr.THETA["3.0"]) > -0.99 > np.cos(rr.THETA["pi-1e-2"])
    cot = rr.cotangent(rr.N_CONV, (3,))
    led = _Ledger()
    for band in bands:
        six = rr.sixd_exact(rr.band_rotvecs(band))
        Rm = rr.rot6d_truth(six)
        rot = Rotation.from_matrix(Rm)
        v64, g64 = _vjp(helper, torch.tensor(six, dtype=torch.float64), torch.tensor(cot, dtype=torch.float64))
        v32, g32 = _vjp(helper, torch.tensor(six), torch.tensor(cot))
        v, g = _vjp(helper, _dev(six), _dev(cot))
        assert v.dtype == torch.float32 and g.dtype == torch.float32
        led.add(band, "geodesic", rr.geodesic(t2n(v), rot), rr.geodesic(v32.numpy(), rot), rr.FLOOR_AA)
        as_mat = rr.max_abs(Rotation.from_rotvec(t2n(v).astype(np.float64)).as_matrix(), Rm)
        _log_measured(f"band {band} | rot6d -> axis-angle helper, as rotation matrices (today's bar: 2e-5 below 3.1 rad, 2e-3 above)", as_mat)
        print(f"helper as rotation matrices, band {band}: {as_mat:.3e}")
        if rr.THETA[band] < 3.1:
            assert as_mat < rr.CAP_HELPER, (band, as_mat)
        led.add(band, "gradient", rr.max_abs(t2n(g), g64.numpy()), rr.max_abs(g32.numpy(), g64.numpy()), _floor_of(g64.numpy()))
        if band == "0":
            assert not t2n(v).any()
    led.check()
