"""Mesh self-intersections without a GPU: the pair rule of include/dposer_hip.h through the fp64 oracle (tests/si_ref.py) on hand cases,
the C struct layout of dposer_mesh_si_args, the exported symbols, and the refusal of CPU tensors."""
import os
import subprocess

import numpy as np
import pytest
import torch

import si_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", sorted(si_ref.hand_cases()))
def test_hand_cases_through_the_oracle(name):
    v, f, want = si_ref.hand_cases()[name]
    flagged, clean, ambiguous = si_ref.classify(v, f)
    assert not ambiguous.any()
    assert np.array_equal(flagged, want) and np.array_equal(clean, ~want)


def test_oracle_is_invariant_under_face_permutation_and_vertex_scale():
    v, f, want = si_ref.hand_cases()["shared_vertex_piercing"]
    assert np.array_equal(si_ref.classify(v, f[::-1].copy())[0], want[::-1])
    assert np.array_equal(si_ref.classify(v * 0.25, f)[0], want)


def test_ring_torus_is_clean_for_the_oracle():
    X, F = si_ref.torus(n_u=24, n_v=20)
    flagged, clean, ambiguous = si_ref.classify(X, F)
    assert clean.all()
    Xs, _ = si_ref.torus(n_u=24, n_v=20, r=1.3)
    assert si_ref.classify(Xs, F)[0].any()


def test_mesh_si_args_struct_matches_the_header_layout(tmp_path):
    """dposer_mesh_si_args as gcc lays it out against its ctypes mirror (the probe of test_smplify_cpu.py)."""
    import ctypes as C
    import shutil
    from dposer_amd import _C
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    cname, ct = "dposer_mesh_si_args", _C.MeshSiArgs
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


def test_mesh_si_symbols_are_exported():
    from dposer_amd import _C
    names = ("dposer_mesh_self_intersections", "dposer_mesh_self_intersections_scratch_bytes")
    for n in names:
        assert n in _C.SIGNATURES
    out = subprocess.check_output(["nm", "-D", "--defined-only", _C.LIB_PATH], text=True)
    syms = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for n in names:
        assert n in syms, n
    l = _C.lib()
    assert l.dposer_mesh_self_intersections_scratch_bytes(500, 13776) >= 216 * 64 * 16 + 500 * 216 * 32
    assert l.dposer_mesh_self_intersections_scratch_bytes(1, 0) == 0


def test_cpu_tensors_are_refused():
    from dposer_amd._C import DPoserHipError
    from dposer_amd.utils.metric import self_intersecting_faces, self_intersections_percentage_hip
    v, f, _ = si_ref.hand_cases()["piercing"]
    with pytest.raises(DPoserHipError):
        self_intersecting_faces(torch.tensor(v[None]), torch.tensor(f))
    with pytest.raises(DPoserHipError):
        self_intersections_percentage_hip(torch.tensor(v[None]), torch.tensor(f))
