"""SMPLify host side without a GPU: the fitting-loss mirror and the time tables against the reference's own values (golden g27), the
host camera helpers, the C struct layout of dposer_smplify_args, and the import boundary of the task module."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _close(a, b, rtol=1e-6, atol=1e-6):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape
    assert np.allclose(a, b, rtol=rtol, atol=atol), float(np.abs(a - b).max())


def test_fitting_losses_match_the_reference_values_and_gradients():
    from dposer_amd.body_model import fitting_losses as fl
    g = load("g27_smplify")
    kp = torch.tensor(g["keypoints"])
    focal, center = torch.tensor(g["focal_length"]), torch.tensor(g["camera_center"])
    const_prior = lambda bp, bt, q: (bp ** 2).sum() / bp.shape[0]
    for tag, prior in (("none", None), ("const", const_prior)):
        jv, bp, bt, ct = (torch.tensor(g[k]).requires_grad_(True) for k in ("lc_joints", "lc_body_pose", "lc_betas", "lc_cam_t"))
        loss = fl.body_fitting_loss(bp, bt, jv, ct, center, kp[:, :, :2], kp[:, :, 2], prior, quan_t=int(g["quan_t"][0]), focal_length=focal,
                                    verbose=False)
        loss.backward()
        # same torch ops in the same order on the same CPU: equal to fp32 rounding of the einsum reductions
        assert abs(loss.item() - float(g[f"lc_body_{tag}_loss"])) <= 1e-6 * abs(float(g[f"lc_body_{tag}_loss"]))
        _close(jv.grad, g[f"lc_body_{tag}_djoints"], rtol=1e-5, atol=1e-9)
        _close(bp.grad, g[f"lc_body_{tag}_dbody_pose"], rtol=1e-5, atol=1e-9)
        _close(bt.grad, g[f"lc_body_{tag}_dbetas"], rtol=1e-5, atol=1e-9)
        with torch.no_grad():
            r = fl.body_fitting_loss(bp, bt, jv, ct, center, kp[:, :, :2], kp[:, :, 2], prior, quan_t=0, focal_length=focal,
                                     output="reprojection", verbose=False)
        _close(r, g[f"lc_body_{tag}_reproj"], rtol=1e-6, atol=1e-6)
    jv, ct = torch.tensor(g["lc_joints"]).requires_grad_(True), torch.tensor(g["lc_cam_t"]).requires_grad_(True)
    loss = fl.camera_fitting_loss(jv, ct, torch.tensor(g["lc_cam_est"]), center, kp[:, :, :2], kp[:, :, 2], focal_length=focal)
    loss.backward()
    assert abs(loss.item() - float(g["lc_cam_loss"])) <= 1e-6 * abs(float(g["lc_cam_loss"]))
    _close(jv.grad, g["lc_cam_djoints"], rtol=1e-5, atol=1e-9)
    # the translation reaches the loss only through the depth term (the projection never reads it)
    _close(ct.grad, g["lc_cam_dcam_t"], rtol=1e-6, atol=0)
    assert (ct.grad[:, :2] == 0).all()


def _schedule(strategy, num_iters, sde_N):
    from dposer_amd.tasks.smplify import SMPLify
    s = object.__new__(SMPLify)
    s.time_strategy, s.num_iters, s.sde_N, s.stages = strategy, num_iters, sde_N, 5
    s.sample_time, s.sample_trun = round(sde_N * 0.9), 20.0
    return s


def test_time_strategy_tables_equal_the_reference():
    g = load("g27_smplify")
    N = int(g["sde_N"])
    s = _schedule("3", int(g["num_iters"]), N)
    assert [s.sample_discrete_time(i) for i in range(5 * int(g["num_iters"]))] == g["quan_t"].tolist()
    for strat in ("2", "3"):
        s = _schedule(strat, 100, N)
        assert [s.sample_discrete_time(i) for i in range(500)] == g[f"quan_t_{strat}_full"].tolist(), strat
    # strategy '1': torch.randint(sde_N, [1]) from the host generator, one draw per iteration and one for the final loss (smplify.py:274)
    s = _schedule("1", 4, N)
    torch.manual_seed(5)
    quan, last = s.time_table()
    torch.manual_seed(5)
    want = [int(torch.randint(N, [1])) for _ in range(21)]
    assert quan + [last] == want


def test_cam_crop2full_and_focal_length():
    from dposer_amd.utils.transforms import cam_crop2full, estimate_focal_length
    rs = np.random.RandomState(3)
    crop = torch.tensor(rs.uniform(0.5, 1.5, (5, 3)), dtype=torch.float32)
    center = torch.tensor(rs.uniform(100, 500, (5, 2)), dtype=torch.float32)
    scale = torch.tensor(rs.uniform(1, 3, 5), dtype=torch.float32)
    shape = torch.tensor([[720, 1280]] * 5, dtype=torch.float32)
    f = estimate_focal_length(shape[:, 0], shape[:, 1])
    assert torch.allclose(f, torch.full((5,), (720. ** 2 + 1280. ** 2) ** 0.5))
    got = cam_crop2full(crop, center, scale, shape, f).double().numpy()
    c, ce, s, fd = crop.double().numpy(), center.double().numpy(), scale.double().numpy(), f.double().numpy()
    bs = s * 200 * c[:, 0] + 1e-9
    want = np.stack([2 * (ce[:, 0] - 640) / bs + c[:, 1], 2 * (ce[:, 1] - 360) / bs + c[:, 2], 2 * fd / bs], 1)
    assert np.allclose(got, want, rtol=1e-5)


def test_smplify_args_struct_matches_the_header_layout(tmp_path):
    """dposer_smplify_args as gcc lays it out against its ctypes mirror (the probe of test_host_cpu.py for the new struct)."""
    import ctypes as C
    import shutil
    from dposer_amd import _C
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    cname, ct = "dposer_smplify_args", _C.SmplifyArgs
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
    assert "dposer_smplify_optimize" in _C.SIGNATURES and "dposer_smplify_scratch_bytes" in _C.SIGNATURES


def test_smplify_module_does_not_import_the_oracle():
    code = "import sys; import dposer_amd.tasks.smplify; print(any(m == 'oracle' or m.startswith('oracle.') for m in sys.modules))"
    out = subprocess.check_output([sys.executable, "-c", code], cwd=ROOT, text=True)
    assert out.strip() == "False"
