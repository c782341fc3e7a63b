"""CPU side of the pose-set distance feature (dposer_pose_set_distances / utils.metric.pose_set_distances, generation_fidelity): the
float64 rule of tests/set_dist_ref.py against the reference's own APD (golden g12) and against a case small enough to check by hand,
the layout of the argument struct, the refusals of the C entries (they run before any launch) and of the Python layer, and the
conditions on the inputs of the GPU test that its index and covered checks rely on."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import set_dist_ref as R
from helpers import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plan(na, nb, J, k):
    from dposer_amd import _C
    out = (C.c_int32 * 4)()
    assert _C.lib().dposer_pose_set_distances_plan(na, nb, J, k, out) == 0
    return tuple(out)


def test_oracle_reproduces_the_reference_apd():
    """golden g12 apd/value is the reference's own average_pairwise_distance (lib/utils/metric.py:8-37) of apd/joints."""
    g = load("g12_likelihood_ode")
    j = g["apd/joints"]
    n = j.shape[0]
    assert abs(R.total(R.distances(j, j)) / (n * (n - 1)) - float(g["apd/value"])) < 1e-6


def test_oracle_on_a_case_checked_by_hand():
    """J = 1, points on a line.  G = {0, 1, 5, 6}, R = {0.5, 2, 2.5, 7, 20}, k = 1.
    Radii (nearest other point of the own set): r_R = (1.5, 0.5, 0.5, 4.5, 13), r_G = (1, 1, 1, 1).
    G against R: 0 -> |0 - 0.5| = 0.5 <= 1.5 only; 1 -> 0.5 <= 1.5 only (|1 - 2| = 1 > 0.5); 5 -> |5 - 7| = 2 <= 4.5 only;
    6 -> 1 <= 4.5 only (|6 - 20| = 14 > 13).  covered = (1, 1, 1, 1): precision 1, density 4 / (1 * 4) = 1.
    R against G (radius 1 everywhere): 0.5 -> both 0 and 1; 2 -> 1 (distance 1); 2.5 -> none (1.5 and 2.5); 7 -> 6; 20 -> none.
    recall = 3 / 5.  coverage: nearest generated point within r_R: 0.5 (0.5 <= 1.5), 2 (1 > 0.5), 2.5 (1.5 > 0.5), 7 (1 <= 4.5),
    20 (14 > 13) -> 2 / 5.  dNN = (0.5 + 0.5 + 2 + 1) / 4 = 1.  APD of G = 2 (1 + 5 + 6 + 4 + 5 + 1) / 12 = 22 / 6."""
    line = lambda xs: np.array([[[x, 0.0, 0.0]] for x in xs], dtype=np.float32)
    G, Rr = line([0, 1, 5, 6]), line([0.5, 2, 2.5, 7, 20])
    assert np.array_equal(R.kth_radius(Rr, 1), [1.5, 0.5, 0.5, 4.5, 13.0]) and np.array_equal(R.kth_radius(G, 1), [1, 1, 1, 1])
    D = R.distances(G, Rr)
    d, idx = R.knn(D, 2)
    assert np.array_equal(idx[:, :2], [[0, 1], [0, 1], [3, 2], [3, 2]])
    assert np.array_equal(d[:, :2], [[0.5, 2], [0.5, 1], [2, 2.5], [1, 3.5]])
    assert np.array_equal(R.covered(D, R.kth_radius(Rr, 1)), [1, 1, 1, 1])
    assert np.array_equal(R.covered(D.T, R.kth_radius(G, 1)), [2, 1, 0, 1, 0])
    f = R.fidelity(G, Rr, 1)
    want = {"APD": 22 / 6, "dNN": 1.0, "precision": 1.0, "recall": 0.6, "density": 1.0, "coverage": 0.4}
    assert set(f) == set(want) and all(abs(f[k] - want[k]) < 1e-12 for k in want), f
    # same set: the own index is left out, an equal pose elsewhere is not; ties go to the smaller index; the tail is +inf / -1
    S = line([3, 1, 3, 1])
    d, idx = R.knn(R.distances(S, S), 4, same_set=True)
    assert np.array_equal(idx[:, :4], [[2, 1, 3, -1], [3, 0, 2, -1], [0, 1, 3, -1], [1, 0, 2, -1]])
    assert np.array_equal(d[:, :4], [[0, 2, 2, np.inf]] * 4)
    assert np.array_equal(R.covered(R.distances(S, S), [0, 0, 1, 2], same_set=True), [2, 1, 2, 1])
    # a NaN reference is never a neighbour and never covers; the sum keeps it
    Rn = Rr.copy()
    Rn[1] = np.nan
    Dn = R.distances(G, Rn)
    assert np.array_equal(R.knn(Dn, 5)[1][:, :5], [[0, 2, 3, 4, -1], [0, 2, 3, 4, -1], [3, 2, 0, 4, -1], [3, 2, 0, 4, -1]])
    assert np.array_equal(R.covered(Dn, [np.inf] * 5), [4, 4, 4, 4]) and np.isnan(R.total(Dn))


def test_set_dist_args_match_the_header_layout(tmp_path):
    """dposer_set_dist_args as the C compiler lays it out against its ctypes mirror and against the offsets the header documents."""
    from dposer_amd import _C
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    cname, ct = "dposer_set_dist_args", _C.SetDistArgs
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dposer_hip.h"', 'int main(void) {',
             f'  printf("size %zu\\n", sizeof({cname}));']
    lines += [f'  printf("{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in ct._fields_]
    lines += ['  return 0;', '}']
    src = tmp_path / "abi_probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "abi_probe"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict((a, int(b)) for a, b in (ln.split() for ln in subprocess.check_output([str(exe)], text=True).splitlines()))
    assert got["size"] == C.sizeof(ct)
    assert [f for f, _ in ct._fields_] == ["a", "b", "na", "nb", "joints", "same_set", "k", "radii", "sum", "knn_dist", "knn_idx", "covered",
                                           "splits", "scratch"]
    for f, _ in ct._fields_:
        assert got[f] == getattr(ct, f).offset, f
    hdr = open(os.path.join(ROOT, "include", "dposer_hip.h")).read()
    body = hdr[hdr.index("typedef struct dposer_set_dist_args {"):hdr.index("} dposer_set_dist_args;")]
    stated = {m.group(1): int(m.group(2)) for m in re.finditer(r"(\w+);\s*/\*\s*(\d+)", body)}
    assert stated == {f: got[f] for f, _ in ct._fields_}
    assert f"sizeof = {got['size']}" in hdr[hdr.index("All-pairs pose-set distances"):]


def test_plan_and_scratch_refusals_and_the_plan_is_a_pure_function():
    from dposer_amd import _C
    lib = _C.lib()
    out = (C.c_int32 * 4)()
    for na, nb, J, k in ((0, 5, 22, 1), (5, 0, 22, 1), (5, 1 << 31, 22, 1), (5, 5, 0, 1), (5, 5, 129, 1), (5, 5, 22, 9), (5, 5, 22, -1),
                         (-3, 5, 22, 1)):
        assert lib.dposer_pose_set_distances_plan(na, nb, J, k, out) == -1 and b"joints" in lib.dposer_last_error(), (na, nb, J, k)
        assert lib.dposer_pose_set_distances_scratch_bytes(na, nb, J, k, 0) == -1
    assert lib.dposer_pose_set_distances_plan(5, 5, 22, 1, None) == -1 and b"NULL" in lib.dposer_last_error()
    assert lib.dposer_pose_set_distances_scratch_bytes(5, 5, 22, 1, -1) == -1
    # the limits themselves pass; na nb may pass 2^32
    for na, nb, J, k in ((1, 1, 1, 0), (1, (1 << 31) - 1, 128, 8), (1 << 20, 1 << 20, 22, 3)):
        assert _plan(na, nb, J, k) == _plan(na, nb, J, k)
        assert lib.dposer_pose_set_distances_scratch_bytes(na, nb, J, k, 0) > 0
    rows, tile, splits, reg = _plan(193, 1031, 22, 3)
    assert rows >= 64 and rows % 64 == 0 and tile >= 1 and splits >= 2 and reg == 1
    assert _plan(193, 1031, 23, 3)[3] == 0 and _plan(193, 1031, 128, 3)[3] == 0 and _plan(193, 1031, 1, 3)[3] == 0
    assert _plan(100, 3, 22, 1)[2] == 1                                            # nothing to split
    # forced splits change the scratch size up to the plan's maximum (one split per tile), not beyond
    by = [lib.dposer_pose_set_distances_scratch_bytes(193, 3 * tile, 22, 3, s) for s in (1, 2, 3, 4, 50)]
    assert by[0] < by[1] < by[2] == by[3] == by[4]
    assert all(b % 256 == 0 for b in by)


def test_entry_refusals_come_before_any_launch():
    """Fake pointers: nothing here touches a device."""
    from dposer_amd import _C
    lib = _C.lib()
    A, U = 0x100000, 0x100002

    def args(**kw):
        base = dict(a=A, b=A + 0x10000, na=10, nb=12, joints=22, same_set=0, k=3, radii=A, sum=A, knn_dist=A, knn_idx=A, covered=A, splits=0,
                    scratch=A)
        base.update(kw)
        return _C.SetDistArgs(**base)

    def rejected(word, **kw):
        rc = lib.dposer_pose_set_distances(C.byref(args(**kw)), None)
        msg = lib.dposer_last_error()
        assert rc == -1 and word in msg, (kw, rc, msg)

    assert lib.dposer_pose_set_distances(None, None) == -1 and b"NULL" in lib.dposer_last_error()
    rejected(b"a is NULL", a=None)
    rejected(b"b is NULL", b=None)
    rejected(b"same_set", same_set=1)                                              # b is another array
    rejected(b"same_set", same_set=1, b=None)                                      # nb != na
    rejected(b"all NULL", sum=None, knn_dist=None, knn_idx=None, covered=None)
    rejected(b"joints", joints=0)
    rejected(b"joints", joints=129)
    rejected(b"joints", na=0)
    rejected(b"joints", nb=1 << 31)
    rejected(b"joints", k=9)
    rejected(b"need 1 <= k", k=0)
    rejected(b"radii", radii=None)
    rejected(b"splits", splits=-1)
    rejected(b"scratch is NULL", scratch=None)
    rejected(b"256-byte", scratch=A + 64)
    rejected(b"4-byte", a=U)
    rejected(b"8-byte", sum=A + 4)


def test_wrappers_refuse_bad_shapes_before_any_device_use_and_cpu_tensors():
    from dposer_amd import _C
    from dposer_amd.utils import metric as M
    a, b = torch.zeros(6, 22, 3), torch.zeros(5, 22, 3)
    for call in (lambda: M.pose_set_distances(torch.zeros(6, 66), k=1), lambda: M.pose_set_distances(torch.zeros(6, 22, 2), k=1),
                 lambda: M.pose_set_distances(torch.zeros(0, 22, 3), k=1), lambda: M.pose_set_distances(torch.zeros(6, 129, 3), k=1),
                 lambda: M.pose_set_distances(a, torch.zeros(5, 21, 3), k=1), lambda: M.pose_set_distances(a, b, k=9),
                 lambda: M.pose_set_distances(a, b, k=-1), lambda: M.pose_set_distances(a, b), lambda: M.pose_set_distances(a, b, k=1, splits=-1),
                 lambda: M.pose_set_distances(a, b, radii=torch.zeros(6)), lambda: M.pose_set_distances(a, radii=torch.zeros(5)),
                 lambda: M.pose_set_distances(a.numpy(), k=1), lambda: M.average_pairwise_distance_hip(torch.zeros(1, 22, 3)),
                 lambda: M.nearest_pose_distance(a, b, k=0), lambda: M.generation_fidelity(a, b, k=0), lambda: M.generation_fidelity(a, b, k=9),
                 lambda: M.generation_fidelity(a, b, k=5), lambda: M.generation_fidelity(torch.zeros(3, 22, 3), a, k=3),
                 lambda: M.generation_fidelity(a, torch.zeros(5, 21, 3), k=3)):
        with pytest.raises(ValueError):
            call()
    for call in (lambda: M.pose_set_distances(a, b, k=1), lambda: M.pose_set_distances(a, want_sum=True),
                 lambda: M.pose_set_distances(a, b, radii=torch.zeros(5)), lambda: M.average_pairwise_distance_hip(a),
                 lambda: M.nearest_pose_distance(a, b), lambda: M.generation_fidelity(a, b, k=3)):
        with pytest.raises(_C.DPoserHipError):
            call()
    # the torch APD is untouched and still runs on CPU tensors
    g = load("g12_likelihood_ode")
    assert abs(float(M.average_pairwise_distance(torch.tensor(g["apd/joints"]))) - float(g["apd/value"])) < 1e-6


def test_gpu_test_inputs_keep_near_ties_and_radius_flips_rare():
    """What tests/test_gpu_set_dist.py relies on, for every case it runs: at most 2 % of the (row, rank <= k) have a float64 gap to the
    next rank below 2 bound(J) (there the index check falls back to a distance check), and at most 2 % of the rows have a covered count
    that differs between radii (1 - bound) and radii (1 + bound) (there the count check is an interval).  A case that breaks a cap gets
    another seed, not another cap."""
    cases = R.gpu_cases(_plan)
    assert {J for _, _, J, _, _ in cases} == {1, 22, 23, 55, 128} and {k for _, _, _, k, _ in cases} == {1, 3, 8}
    assert {_plan(na, nb, J, k)[3] for na, nb, J, k, _ in cases} == {0, 1}                    # both paths
    assert any(_plan(na, nb, J, k)[2] >= 2 for na, nb, J, k, _ in cases)
    assert any(na == 1 for na, *_ in cases) and any(nb == 1 for _, nb, *_ in cases)
    for na, nb, J, k, seed in cases:
        a, b = R.make_sets(na, nb, J, seed)
        D = R.distances(a, b)
        ties, flips = R.near_tie_share(D, k, J), R.covered_flip_share(D, R.case_radii(b), J)
        print(f"case {(na, nb, J, k, seed)}: near-tie share {ties:.4f}, covered flip share {flips:.4f}")
        assert ties <= 0.02 and flips <= 0.02, (na, nb, J, k, seed)
