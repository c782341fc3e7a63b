"""CPU side of the data feed (csrc/feed.hip, dataset/feed.py): the permutation rule as tests/feed_ref.py states it is a bijection that
changes with epoch and seed and looks random where that can be counted, the step -> (epoch, base, rank slice) arithmetic of DeviceFeed, the
C struct layout of dposer_batch_gather_args and the exported symbol."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import feed_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 2, 3, 5, 63, 64, 65, 1000, 4097, 65537)
# The seed of the statistical checks below.  It was not tuned: it is the first one tried, and the only requirement ever put on it is that
# the mirror passes with it (the outcome is deterministic).
SEED = 20240229


@pytest.mark.parametrize("N", SIZES)
def test_permutation_is_a_bijection(N):
    for epoch in (0, 1, 7):
        p = feed_ref.permute(np.arange(N), N, SEED, epoch)
        assert p.dtype == np.int64 and p.shape == (N,)
        assert np.array_equal(np.sort(p), np.arange(N)), (N, epoch)


def test_epochs_and_seeds_give_different_permutations():
    N = 1000
    a = feed_ref.permute(np.arange(N), N, SEED, 0)
    assert not np.array_equal(a, feed_ref.permute(np.arange(N), N, SEED, 1))
    assert not np.array_equal(a, feed_ref.permute(np.arange(N), N, SEED + 1, 0))
    assert not np.array_equal(a, feed_ref.permute(np.arange(N), N, SEED + (1 << 32), 0))      # the high key word counts too
    assert np.array_equal(a, feed_ref.permute(np.arange(N), N, SEED, 0))                      # and it is a function


def test_first_element_takes_every_value_over_the_epochs():
    """N = 16, 256 epochs: a true random permutation misses one of the 16 values with chance about 16 (15/16)^256 = 1e-6."""
    first = {int(feed_ref.permute(np.array([0]), 16, SEED, e)[0]) for e in range(256)}
    assert first == set(range(16))


def test_fixed_points_are_poisson():
    """N = 1000: the fixed points of a random permutation are Poisson(1), so their sum over 64 epochs has mean 64 and sigma 8; the bound
    is +- 5 sigma.  Deterministic for the committed seed (see SEED)."""
    N = 1000
    total = sum(int((feed_ref.permute(np.arange(N), N, SEED, e) == np.arange(N)).sum()) for e in range(64))
    print("fixed points over 64 epochs:", total)
    assert 24 <= total <= 104


def test_half_bits_rule():
    assert [feed_ref.half_bits(n) for n in (1, 2, 3, 4, 5, 16, 17, 64, 65, 1 << 20, (1 << 20) + 1, 1 << 62)] == \
        [1, 1, 1, 1, 2, 2, 3, 3, 4, 10, 11, 31]
    for n in SIZES:
        assert n <= 1 << (2 * feed_ref.half_bits(n)) and (1 << (2 * feed_ref.half_bits(n))) <= max(4, 4 * n - 1)     # domain below 4 N


def test_step_arithmetic_and_rank_shards():
    from dposer_amd.dataset.feed import feed_position, feed_steps_per_epoch
    N, B = 1000, 24
    assert feed_steps_per_epoch(N, B) == 41 and feed_steps_per_epoch(N, B, 2) == 20 and feed_steps_per_epoch(48, B, 2) == 1   # drop_last
    with pytest.raises(ValueError, match="global batch"):
        feed_steps_per_epoch(47, B, 2)
    with pytest.raises(ValueError):
        feed_steps_per_epoch(B - 1, B)
    spe2 = feed_steps_per_epoch(N, B, 2)
    assert spe2 == feed_steps_per_epoch(N, 2 * B, 1)
    for step in (0, 1, spe2 - 1, spe2, 3 * spe2 + 7):
        whole = feed_position(step, spe2, 2 * B)
        assert whole == feed_ref.position(step, spe2, 2 * B) == (step // spe2, (step % spe2) * 2 * B)
        halves = []
        for r in (0, 1):
            epoch, base = feed_position(step, spe2, B, 2, r)
            assert (epoch, base) == feed_ref.position(step, spe2, B, 2, r) == (whole[0], whole[1] + r * B)
            assert base + B <= N
            halves.append(feed_ref.permute(np.arange(base, base + B), N, SEED, epoch))
        assert not set(halves[0]) & set(halves[1])                                              # disjoint shards ...
        assert np.array_equal(np.concatenate(halves), feed_ref.indices(step, N, 2 * B, SEED))   # ... that tile the W = 1 batch of 2 B
    # one epoch of the two ranks together visits steps_per_epoch * 2 B distinct rows; the tail of the permutation is unused
    seen = np.concatenate([feed_ref.indices(s, N, B, SEED, 2, r) for s in range(spe2) for r in (0, 1)])
    assert len(set(seen.tolist())) == spe2 * 2 * B == 960


def test_device_feed_refuses_bad_input_before_it_needs_a_gpu():
    from dposer_amd._C import DPoserHipError
    from dposer_amd.dataset.feed import DeviceFeed
    x = torch.zeros(100, 63)
    for bad in (x.double(), x.half(), x[0], x[None], torch.zeros(0, 63)):
        with pytest.raises(ValueError, match="float32"):
            DeviceFeed(bad, 10, num_replicas=1, rank=0)
    with pytest.raises(ValueError, match="float32"):
        DeviceFeed(x, 10, shapes=torch.zeros(100, 10, dtype=torch.float64), num_replicas=1, rank=0)
    with pytest.raises(ValueError, match="fewer"):
        DeviceFeed(x, 10, shapes=torch.zeros(99, 10), num_replicas=1, rank=0)
    with pytest.raises(ValueError, match="global batch"):
        DeviceFeed(x, 51, num_replicas=2, rank=0)
    with pytest.raises(ValueError, match="rank"):
        DeviceFeed(x, 10, num_replicas=2, rank=2)
    if not torch.cuda.is_available():
        with pytest.raises(DPoserHipError, match="no CPU fallback"):
            DeviceFeed(x, 10, num_replicas=1, rank=0)


def test_batch_gather_symbol_struct_and_stream_id(tmp_path):
    from dposer_amd import _C
    from oracle import philox
    hdr = open(os.path.join(ROOT, "include", "dposer_hip.h")).read()
    assert "dposer_batch_gather(" in hdr and "Permutation rule" in hdr and "dposer_batch_gather" in _C.SIGNATURES
    for path in (_C.LIB_PATH, os.path.join(os.path.dirname(_C.LIB_PATH), "libdposer_hip_testhooks.so")):
        assert hasattr(C.CDLL(path), "dposer_batch_gather"), path
    # the stream id of the feed: rng.h and the mirror agree, and no other stream of rng.h / oracle/philox.py has it
    rng = open(os.path.join(ROOT, "dposer_amd", "csrc", "rng.h")).read()
    ids = {k: int(v) for k, v in re.findall(r"(STREAM_[A-Z0-9_]+)\s*=\s*(\d+)", rng)}
    assert ids["STREAM_FEED"] == feed_ref.STREAM_FEED
    others = {v for k, v in ids.items() if k != "STREAM_FEED"} | {v for k, v in vars(philox).items() if k.startswith("STREAM_")}
    others |= {ids["STREAM_DROPOUT0"] + site for site in range(8)}
    assert feed_ref.STREAM_FEED not in others
    # an argument error comes back as a code and a message, before anything is launched (no GPU needed)
    a = _C.BatchGatherArgs()
    a.N, a.B, a.base = 10, 4, 7
    a.indices = 0x1000
    assert _C.lib().dposer_batch_gather(C.byref(a), None) < 0 and b"base + B" in _C.lib().dposer_last_error()
    a.base, a.indices = 0, None
    assert _C.lib().dposer_batch_gather(C.byref(a), None) < 0 and b"all NULL" in _C.lib().dposer_last_error()
    assert _C.lib().dposer_batch_gather(None, None) < 0
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dposer_hip.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(dposer_batch_gather_args));']
    lines += [f'  printf("{f} %zu\\n", offsetof(dposer_batch_gather_args, {f}));' for f, _ in _C.BatchGatherArgs._fields_]
    lines += ['  return 0;', '}']
    (tmp_path / "probe.c").write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(tmp_path / "probe.c"), "-o", str(tmp_path / "probe")])
    got = dict(ln.split() for ln in subprocess.check_output([str(tmp_path / "probe")], text=True).splitlines())
    assert int(got["size"]) == C.sizeof(_C.BatchGatherArgs)
    for f, _ in _C.BatchGatherArgs._fields_:
        assert int(got[f]) == getattr(_C.BatchGatherArgs, f).offset, f
