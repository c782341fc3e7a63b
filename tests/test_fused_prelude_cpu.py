"""CPU checks of the prelude the one-call task paths share (dposer_amd/tasks/_fused.py): the normaliser tables handed to the kernels and
the host float arrays.  No GPU and no library: a stub normaliser with the four statistics tables."""
import ctypes as C

import pytest
import torch

from dposer_amd.tasks._fused import float_array, normalizer_tables


class _StubNormalizer:
    """The attributes of dataset.AMASS.Posenormalizer that the prelude reads; the tables shaped [1, D] as a saved statistics file has them."""

    def __init__(self, rot_rep, normalize=True, min_max=True):
        self.rot_rep, self.normalize, self.min_max = rot_rep, normalize, min_max
        D = 21 * (3 if rot_rep == "axis" else 6)
        g = torch.Generator().manual_seed(D)
        t = lambda: torch.randn(1, D, generator=g, dtype=torch.float64)
        self.min_poses, self.max_poses, self.mean_poses, self.std_poses = t(), t(), t(), t()


@pytest.mark.parametrize("rot_rep", ["axis", "rot6d"])
def test_no_normalisation_is_mode_0_without_tables(rot_rep):
    nz = _StubNormalizer(rot_rep, normalize=False)
    assert normalizer_tables(nz, torch.zeros(4, 63)) == (0, None, None)


@pytest.mark.parametrize("rot_rep,D", [("axis", 63), ("rot6d", 126)])
@pytest.mark.parametrize("min_max", [False, True])
def test_tables_are_the_modes_pair_flat_contiguous_float32(rot_rep, D, min_max):
    nz = _StubNormalizer(rot_rep, min_max=min_max)
    like = torch.zeros(5, 63)
    mode, a, b = normalizer_tables(nz, like)
    assert mode == (2 if min_max else 1)
    want_a, want_b = (nz.min_poses, nz.max_poses) if min_max else (nz.mean_poses, nz.std_poses)
    for got, want in ((a, want_a), (b, want_b)):
        assert got.dtype == torch.float32 and got.dim() == 1 and got.numel() == D and got.is_contiguous()
        assert got.device == like.device
        assert torch.equal(got, want.reshape(-1).float())


def test_tables_of_a_strided_source_come_back_contiguous():
    nz = _StubNormalizer("axis", min_max=False)
    wide = torch.arange(126, dtype=torch.float32).reshape(1, 126)
    nz.mean_poses, nz.std_poses = wide[:, ::2], wide[:, 1::2]
    mode, a, b = normalizer_tables(nz, torch.zeros(2, 63))
    assert mode == 1 and a.is_contiguous() and b.is_contiguous()
    assert torch.equal(a, torch.arange(0, 126, 2, dtype=torch.float32)) and torch.equal(b, torch.arange(1, 126, 2, dtype=torch.float32))


def test_float_array_keeps_values_and_length():
    xs = [0.5, -1.25, 3.0, 1e-3]
    arr = float_array(xs)
    assert len(arr) == 4 and arr._type_ is C.c_float
    assert list(arr) == [C.c_float(x).value for x in xs]
    assert list(float_array(x * 2 for x in (1, 2, 3))) == [2.0, 4.0, 6.0]          # a generator, as the schedules are passed
    assert list(float_array(torch.tensor([0.25, 0.75]))) == [0.25, 0.75]           # tensor entries (the time grid)


def test_float_array_of_nothing_still_has_one_slot():
    arr = float_array([])
    assert len(arr) == 1 and arr._type_ is C.c_float and arr[0] == 0.0
