"""numpy statement of the data feed's permutation rule (include/dposer_hip.h, "Permutation rule" of dposer_batch_gather; kernel in
dposer_amd/csrc/feed.hip), built on oracle/philox.py.  TEST INFRASTRUCTURE: the product never imports it.

    pi(seed, epoch, p): balanced 4-round Feistel network on k = max(2, 2 ceil(ceil(log2 N) / 2)) bits, round function
    Philox4x32-10(counter = (R, epoch, STREAM_FEED, round), key = seed) word 0 masked to k / 2 bits, cycle-walked until the value is < N.
"""
from __future__ import annotations

import numpy as np

from oracle.philox import philox4x32_10

STREAM_FEED = 8             # dposer_amd/csrc/rng.h
ROUNDS = 4


def half_bits(N):
    bits = 0 if N <= 1 else int(N - 1).bit_length()          # ceil(log2 N)
    return max(2, 2 * ((bits + 1) // 2)) // 2


def feistel(x, h, seed, epoch):
    """One pass of the network over uint64 values x < 2^(2h)."""
    mask = np.uint32((1 << h) - 1)
    L = (x >> np.uint64(h)).astype(np.uint32)
    R = x.astype(np.uint32) & mask
    for r in range(ROUNDS):
        F = philox4x32_10(R, np.uint32(epoch), np.uint32(STREAM_FEED), np.uint32(r), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)[0] & mask
        L, R = R, L ^ F
    return (L.astype(np.uint64) << np.uint64(h)) | R.astype(np.uint64)


def permute(positions, N, seed, epoch):
    """pi(seed, epoch, positions) as int64; positions in [0, N)."""
    x = np.asarray(positions, dtype=np.uint64).reshape(-1).copy()
    assert x.size == 0 or int(x.max()) < N
    h = half_bits(N)
    todo = np.ones(x.shape, dtype=bool)
    while todo.any():
        x[todo] = feistel(x[todo], h, seed, epoch)
        todo &= x >= np.uint64(N)
    return x.astype(np.int64)


def position(step, steps_per_epoch, B, W=1, rank=0):
    """(epoch, base) of a step: the arithmetic DeviceFeed states in its docstring, written independently."""
    return step // steps_per_epoch, (step % steps_per_epoch) * W * B + rank * B


def indices(step, N, B, seed, W=1, rank=0):
    spe = N // (W * B)
    epoch, base = position(step, spe, B, W, rank)
    return permute(np.arange(base, base + B), N, seed, epoch)
