"""CPU tests of the few-step sampler's host side: the time grids (``dpm_time_grid``), the coefficient schedule of
``dposer_dpm_coefficients`` against the float64 statement in tests/dpm_ref.py, that statement against the reference-pinned
``oracle.score_ref.multi_step_denoise`` (its first-order member), the observed convergence order on an analytic Gaussian score with the
library's own coefficients, and the argument checks.  No GPU is needed: the coefficient entry is host code."""
import math

import numpy as np
import pytest
import torch

import dpm_ref
from oracle import score_ref as R
from weights import make_weights

KINDS = ("subvp", "vp", "ve")


def _sdes(kind):
    """(the library's SDE object, the oracle's)."""
    from dposer_amd.algorithms.advanced import sde_lib
    if kind == "ve":
        return sde_lib.VESDE(0.01, 50.0, 1000), R.VE()
    if kind == "vp":
        return sde_lib.VPSDE(0.1, 20.0, 1000), R.VP()
    return sde_lib.subVPSDE(0.1, 20.0, 1000), R.SubVP()


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)) / np.maximum(np.abs(np.asarray(b)), 1e-300)))


# ---- grids ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_log_snr_grid_is_uniform_in_lambda_with_exact_end_points(kind):
    from dposer_amd.algorithms.advanced.sampling import dpm_time_grid
    sde, so = _sdes(kind)
    ts = dpm_time_grid(sde, 16, "logSNR", 1e-3)
    assert ts.dtype == np.float64 and ts.shape == (17,)
    assert ts[0] == 1.0 and ts[-1] == 1e-3
    lam = np.array([dpm_ref.log_snr(so, t) for t in ts])
    want = np.linspace(lam[0], lam[-1], 17)
    dev = float(np.max(np.abs(lam - want)) / np.max(np.abs(want)))
    print(f"[{kind}] logSNR grid: max deviation from uniform, relative to max |lambda|: {dev:.2e}")
    assert dev < 1e-9
    step = np.diff(lam)
    assert float(np.max(np.abs(step - step.mean())) / abs(step.mean())) < 1e-9 * 17


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("skip_type", ["logSNR", "time_uniform", "time_quadratic"])
def test_grids_decrease_strictly_and_end_exactly(kind, skip_type):
    from dposer_amd.algorithms.advanced.sampling import dpm_time_grid
    sde, _ = _sdes(kind)
    for steps, eps, T in ((1, 1e-3, None), (6, 1e-3, None), (20, 1e-5, None), (7, 1e-2, 0.5)):
        ts = dpm_time_grid(sde, steps, skip_type, eps, T)
        assert ts.shape == (steps + 1,) and ts.dtype == np.float64
        assert ts[0] == (1.0 if T is None else T) and ts[-1] == eps
        assert np.all(np.diff(ts) < 0)
        assert np.all(np.diff(ts.astype(np.float32)) < 0)          # also as the fp32 times the sampler call takes
    if skip_type == "time_uniform":
        assert np.allclose(np.diff(dpm_time_grid(sde, 8, skip_type, 1e-3)), -(1.0 - 1e-3) / 8, rtol=1e-12)
    if skip_type == "time_quadratic":
        assert np.allclose(np.diff(np.sqrt(dpm_time_grid(sde, 8, skip_type, 1e-3))), -(1.0 - math.sqrt(1e-3)) / 8, rtol=1e-9)


def test_grid_refuses_what_it_does_not_know():
    from dposer_amd.algorithms.advanced.sampling import dpm_time_grid
    sde, _ = _sdes("vp")
    with pytest.raises(ValueError):
        dpm_time_grid(sde, 8, "cosine", 1e-3)
    with pytest.raises(ValueError):
        dpm_time_grid(sde, 0, "logSNR", 1e-3)
    with pytest.raises(ValueError):
        dpm_time_grid(sde, 8, "logSNR", 2.0)


# ---- schedule ------------------------------------------------------------------------------------------------------------------------
def _nonuniform(n):
    """n + 1 decreasing times with uneven steps in time and in log-SNR."""
    rs = np.random.RandomState(100 + n)
    w = np.cumsum(rs.uniform(0.3, 1.7, n))
    return np.concatenate([[1.0], 1.0 - (1.0 - 2e-3) * w / w[-1]])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("lof", [True, False])
@pytest.mark.parametrize("n", [1, 2, 6])
def test_coefficients_match_the_float64_statement(kind, order, lof, n):
    from dposer_amd.algorithms.advanced.sampling import dpm_coefficients, dpm_time_grid
    sde, so = _sdes(kind)
    for times in (dpm_time_grid(sde, n, "logSNR", 1e-3), dpm_time_grid(sde, n, "time_uniform", 1e-3), _nonuniform(n)):
        got = dpm_coefficients(sde, times, order, lof)
        want = dpm_ref.coefficients(so, times, order, lof)
        assert got.shape == (n, 3) and got.dtype == np.float64
        for i in range(n):
            eff = dpm_ref.effective_order(order, lof, i, n)
            assert (got[i, 2] != 0.0) == (eff == 2), (i, got[i])
        err = _rel(got[want != 0], want[want != 0])
        print(f"[{kind} order {order} lof {lof} n {n}] coefficients: max relative difference {err:.2e}")
        assert err < 1e-12
        assert np.all(got[want == 0] == 0.0)


def test_effective_order_pattern():
    """order 2, n = 6: start-up step at order 1, second-order middle, the last step at order 1 only with lower_order_final."""
    from dposer_amd.algorithms.advanced.sampling import dpm_coefficients, dpm_time_grid
    sde, _ = _sdes("subvp")
    ts = dpm_time_grid(sde, 6, "logSNR", 1e-3)
    assert [c != 0.0 for c in dpm_coefficients(sde, ts, 2, True)[:, 2]] == [False, True, True, True, True, False]
    assert [c != 0.0 for c in dpm_coefficients(sde, ts, 2, False)[:, 2]] == [False, True, True, True, True, True]
    assert not dpm_coefficients(sde, ts, 1, True)[:, 2].any()
    a, b = dpm_coefficients(sde, ts, 2, True), dpm_coefficients(sde, ts, 2, False)
    assert np.array_equal(a[:5], b[:5])                            # lower_order_final changes only the last step
    assert np.array_equal(a[5, :1], b[5, :1]) and a[5, 1] != b[5, 1]


# ---- the float64 statement against the reference-pinned oracle ------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_order_one_is_multi_step_denoise(kind):
    """dpm_ref at order 1 on linear_interpolation(t, t / 20, 11) is R.multi_step_denoise(N = 10): algebraically the same update."""
    _, so = _sdes(kind)
    p = {k: v.double() for k, v in make_weights(31).items()}
    p["sigmas"] = R.sigma_table().double()
    rs = np.random.RandomState(5)
    B = 6
    x_t = torch.tensor(rs.standard_normal((B, 63)) * (20.0 if kind == "ve" else 1.0), dtype=torch.float64)
    t = torch.full((B,), 0.6, dtype=torch.float64)
    _, est = R.multi_step_denoise(p, so, x_t, t, t / 20, 10)
    alpha_w = torch.linspace(0, 1, 11)[:, None]                    # (misc.py:58-61, as multi_step_denoise forms its grid)
    times = ((1 - alpha_w) * t + alpha_w * (t / 20))[:, 0].numpy()
    _, x, _ = dpm_ref.dpm_sampler(p, so, x_t, times, 1)
    err = float(torch.linalg.norm(x - est) / torch.linalg.norm(est))
    print(f"[{kind}] order-1 solver vs multi_step_denoise, rel-L2: {err:.2e}")
    assert err < 1e-10


# ---- observed order on an analytic score, with the library's coefficients ---------------------------------------------------------------
def _gauss_error(kind, order, n, c=0.5, eps=1e-3):
    """x_0 ~ N(0, c^2): D(x, t) = alpha c^2 x / (alpha^2 c^2 + sigma^2); the probability-flow solution from T to eps is
    x(T) sqrt(alpha_eps^2 c^2 + sigma_eps^2) / sqrt(alpha_T^2 c^2 + sigma_T^2).  Relative error of the solver's end point."""
    from dposer_amd.algorithms.advanced.sampling import dpm_coefficients, dpm_time_grid
    sde, so = _sdes(kind)
    ts = dpm_time_grid(sde, n, "logSNR", eps)
    coef = dpm_coefficients(sde, ts, order, True)
    x, d_prev = 1.0, 0.0
    for i in range(n):
        a, s = dpm_ref.alpha_sigma(so, ts[i])
        d = a * c * c * x / (a * a * c * c + s * s)
        x, d_prev = coef[i, 0] * x + coef[i, 1] * d + coef[i, 2] * d_prev, d
    a0, s0 = dpm_ref.alpha_sigma(so, ts[0])
    a1, s1 = dpm_ref.alpha_sigma(so, ts[-1])
    exact = math.sqrt(a1 * a1 * c * c + s1 * s1) / math.sqrt(a0 * a0 * c * c + s0 * s0)
    return abs(x - exact) / exact


@pytest.mark.parametrize("kind", KINDS)
def test_observed_order_on_a_gaussian_score(kind):
    e1 = {n: _gauss_error(kind, 1, n) for n in (32, 64)}
    e2 = {n: _gauss_error(kind, 2, n) for n in (32, 64)}
    r1, r2 = e1[32] / e1[64], e2[32] / e2[64]
    print(f"[{kind}] order 1: errors {e1[32]:.3e} -> {e1[64]:.3e}, ratio {r1:.2f};  order 2: {e2[32]:.3e} -> {e2[64]:.3e}, ratio {r2:.2f};"
          f"  order 2 / order 1 at n = 64: 1/{e1[64] / e2[64]:.1f}")
    assert 1.8 <= r1 <= 2.2
    assert 3.5 <= r2 <= 4.5
    assert e2[64] <= e1[64] / 10


# ---- argument checks -------------------------------------------------------------------------------------------------------------------
def test_coefficient_entry_refuses_bad_arguments():
    from dposer_amd import _C
    from dposer_amd.algorithms.advanced import sde_lib
    from dposer_amd.algorithms.advanced.sampling import dpm_coefficients
    sde, _ = _sdes("subvp")
    good = np.array([1.0, 0.5, 0.1, 1e-3])
    assert dpm_coefficients(sde, good, 2).shape == (3, 3)
    for times, order, what in ((np.array([1.0, 0.5, 0.6, 1e-3]), 2, "decreasing"), (np.array([1.0, 0.5, 0.5, 1e-3]), 1, "decreasing"),
                               (np.array([1.5, 0.5, 1e-3]), 1, "T]"), (np.array([1.0, 0.5, 0.0]), 1, "(0"), (np.array([1.0, 0.5, float("nan")]), 1, "(0"),
                               (good, 3, "order"), (good, 0, "order"), (np.array([1.0]), 2, "n_steps")):
        with pytest.raises(_C.DPoserHipError, match="code -1") as ei:
            dpm_coefficients(sde, times, order)
        assert what in str(ei.value), (what, str(ei.value))
    for disc in (sde_lib.VPSDE(0.1, 20.0, 1000), sde_lib.VESDE(0.01, 50.0, 1000)):      # the two discrete score-function kinds
        with pytest.raises(_C.DPoserHipError, match="code -2"):
            dpm_coefficients(disc, good, 2, continuous=False)
    assert b"continuous" in _C.lib().dposer_last_error()
