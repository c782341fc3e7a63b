"""dposer_batch_gather / DeviceFeed on the GPU (csrc/feed.hip, dataset/feed.py) against the numpy statement of the permutation rule
(tests/feed_ref.py): the indices exactly, the gathered rows bit for bit and inside their buffers, a whole epoch, the rank shards, one case
whose element offsets pass 2^31, and the argument errors."""
import numpy as np
import pytest
import torch

import feed_ref
from gpu_common import DEV

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 3, 5, 63, 64, 65, 1000, 4097, 65537)
SEED = 0x5EED0123456789AB                  # both key words in use


def _feed(N, D, B, **kw):
    from dposer_amd.dataset.feed import DeviceFeed
    gen = torch.Generator().manual_seed(N * 131 + D)
    data = torch.randn(N, D, generator=gen)
    kw.setdefault("seed", SEED)
    kw.setdefault("num_replicas", 1)
    kw.setdefault("rank", 0)
    return DeviceFeed(data, B, **kw), data


@pytest.mark.parametrize("N", SIZES)
def test_indices_equal_the_mirror(N):
    for B in (1, 63, 64, 65):
        if B > N:
            continue
        feed, _ = _feed(N, 3, B)
        spe = N // B
        assert feed.steps_per_epoch == spe == len(feed)
        for step in sorted({0, spe // 2, spe - 1, spe, 7 * spe + spe // 2}):                    # start, middle, last of an epoch, first of the next
            got = feed.indices(step)
            assert got.dtype == torch.int64 and got.shape == (B,) and got.is_cuda
            want = feed_ref.indices(step, N, B, SEED)
            assert np.array_equal(got.cpu().numpy(), want), (N, B, step)
            assert feed.epoch_of(step) == step // spe


def _guarded(shape, dtype, fill):
    """A tensor of ``shape`` in the middle of a buffer of guard words; (view, buffer, lo, hi)."""
    n = int(np.prod(shape))
    guard = 4096
    buf = torch.full((n + 2 * guard,), fill, dtype=dtype, device=DEV)
    return buf[guard:guard + n].view(shape), buf, guard, guard + n


@pytest.mark.parametrize("D", (1, 63, 64, 67, 126))
@pytest.mark.parametrize("with_aux", (False, True))
def test_gathered_rows_are_bit_equal_and_stay_inside_their_buffers(D, with_aux):
    N, D_aux = 1000, 10
    shapes = torch.randn(N + 7, D_aux, generator=torch.Generator().manual_seed(5)) if with_aux else None
    for B in (1, 63, 64, 65):
        feed, data = _feed(N, D, B, shapes=shapes)
        for step in (0, N // B - 1, N // B + 2):
            epoch, base = feed.position(step)
            want = feed_ref.permute(np.arange(base, base + B), N, SEED, epoch)
            out, obuf, olo, ohi = _guarded((B, D), torch.float32, -7.25)
            idx, ibuf, ilo, ihi = _guarded((B,), torch.int64, -99)
            aux, abuf, alo, ahi = _guarded((B, D_aux), torch.float32, -7.25) if with_aux else (None, None, 0, 0)
            feed.gather(epoch, base, B, out=out, aux_out=aux, indices=idx)
            torch.cuda.synchronize()
            assert np.array_equal(idx.cpu().numpy(), want)
            assert torch.equal(out.cpu(), data[want]), (D, B, step)                              # bit-equal (torch.equal on fp32 payloads)
            assert np.array_equal(out.cpu().numpy().view(np.uint32), data[want].numpy().view(np.uint32))
            assert bool((obuf[:olo] == -7.25).all()) and bool((obuf[ohi:] == -7.25).all())
            assert bool((ibuf[:ilo] == -99).all()) and bool((ibuf[ihi:] == -99).all())
            if with_aux:
                assert torch.equal(aux.cpu(), shapes[want])
                assert bool((abuf[:alo] == -7.25).all()) and bool((abuf[ahi:] == -7.25).all())
            got = feed.batch(step)
            if with_aux:
                assert set(got) == {"poses", "shapes"} and torch.equal(got["poses"], out) and torch.equal(got["shapes"], aux)
            else:
                assert torch.equal(got, out)


def test_one_epoch_visits_every_row_once():
    N, B = 4096, 64
    feed, data = _feed(N, 63, B)
    assert feed.steps_per_epoch == 64
    for first in (0, 64 * 3):                                                                   # epoch 0 and epoch 3
        idx = torch.cat([feed.indices(first + s) for s in range(64)])
        assert torch.equal(torch.sort(idx).values, torch.arange(N, device=DEV))
        rows = torch.cat([feed.batch(first + s) for s in range(64)])
        assert torch.equal(rows, data.to(DEV)[idx])
    assert not torch.equal(feed.indices(0), feed.indices(64))                                   # the next epoch is another permutation


def test_two_rank_feeds_reproduce_the_halves_of_the_global_batch():
    N, B = 4097, 64
    whole, data = _feed(N, 63, 2 * B)
    r0, _ = _feed(N, 63, B, num_replicas=2, rank=0)
    r1, _ = _feed(N, 63, B, num_replicas=2, rank=1)
    assert whole.steps_per_epoch == r0.steps_per_epoch == r1.steps_per_epoch == N // (2 * B)
    for step in (0, 5, whole.steps_per_epoch - 1, whole.steps_per_epoch, 3 * whole.steps_per_epoch + 1):
        w = whole.batch(step)
        assert torch.equal(r0.batch(step), w[:B]) and torch.equal(r1.batch(step), w[B:])
        wi = whole.indices(step)
        assert torch.equal(torch.cat([r0.indices(step), r1.indices(step)]), wi) and wi.unique().numel() == 2 * B


def test_row_offsets_past_two_billion_elements():
    """N D = (2^25 + 3) 66 = 2.2e9 elements (8.9 GB): the rows the mirror names, and only they, carry a sentinel (512 rows of eight steps, some
    of them at element offsets past 2^31); every batch must come back with its rows' sentinels."""
    from dposer_amd.dataset.feed import DeviceFeed
    N, D, B = (1 << 25) + 3, 66, 64
    data = torch.zeros(N, D, device=DEV)
    assert data.numel() > 2 ** 31
    feed = DeviceFeed(data, B, seed=SEED, num_replicas=1, rank=0)
    assert feed.poses.data_ptr() == data.data_ptr()                                             # no second copy of 8.9 GB
    spe = feed.steps_per_epoch
    steps = (0, 1, 2, 3, spe // 2, spe - 1, spe, spe + 3)
    want = {s: feed_ref.indices(s, N, B, SEED) for s in steps}
    allrows = np.concatenate(list(want.values()))
    # both sides of the 32-bit line: 3 % of the rows lie past it, 13 of these 512 by the mirror
    assert (allrows * D > 2 ** 31).sum() >= 8 and (allrows * D < 2 ** 31).sum() >= 8 and len(set(allrows.tolist())) == len(allrows)
    rows = torch.tensor(allrows, device=DEV)
    data[rows] = (rows % 8191)[:, None].float() + torch.arange(D, device=DEV)[None, :].float() / 128 + 1.0    # exact in fp32
    for s in steps:
        assert np.array_equal(feed.indices(s).cpu().numpy(), want[s]), s
        got = feed.batch(s).cpu()
        w = torch.tensor(want[s])
        expect = (w % 8191)[:, None].float() + torch.arange(D)[None, :].float() / 128 + 1.0
        assert torch.equal(got, expect), s
    del data, feed
    torch.cuda.empty_cache()


def test_argument_errors():
    from dposer_amd._C import DPoserHipError
    from dposer_amd.dataset.feed import DeviceFeed
    feed, data = _feed(100, 63, 10)
    out = torch.empty(10, 63, device=DEV)
    with pytest.raises(DPoserHipError, match="base \\+ B"):
        feed.gather(0, 91, 10, out=out)
    with pytest.raises(DPoserHipError, match="base \\+ B"):
        feed.gather(0, -1, 10, out=out)
    with pytest.raises(DPoserHipError, match="all NULL"):
        feed.gather(0, 0, 10)
    with pytest.raises(DPoserHipError, match="no CPU fallback"):
        feed.gather(0, 0, 10, out=torch.empty(10, 63))
    with pytest.raises(DPoserHipError, match="no CPU fallback"):
        feed.gather(0, 0, 10, indices=torch.empty(10, dtype=torch.int64))
    with pytest.raises(ValueError, match="float32"):
        feed.gather(0, 0, 10, out=torch.empty(10, 63, device=DEV, dtype=torch.float64))
    with pytest.raises(ValueError, match="int64"):
        feed.gather(0, 0, 10, indices=torch.empty(10, device=DEV, dtype=torch.int32))
    with pytest.raises(ValueError):
        feed.gather(0, 0, 10, out=torch.empty(10, 64, device=DEV))
    with pytest.raises(ValueError, match="no shapes"):
        feed.gather(0, 0, 10, aux_out=torch.empty(10, 10, device=DEV))
    with pytest.raises(ValueError, match="float32"):
        DeviceFeed(data.to(DEV).double(), 10, num_replicas=1, rank=0)
    with pytest.raises(ValueError, match="float32"):
        DeviceFeed(data.to(DEV)[0], 10, num_replicas=1, rank=0)
    with pytest.raises(ValueError, match="global batch"):
        DeviceFeed(data, 51, num_replicas=2, rank=0)
    feed.gather(0, 90, 10, out=out)                                                             # base + B == N is the last legal batch
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), data[feed_ref.permute(np.arange(90, 100), 100, SEED, 0)])
