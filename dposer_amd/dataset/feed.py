"""Device-resident shuffled data feed: what run/train.py:70-93 builds as ``DataLoader(dataset, batch_size, shuffle=True, drop_last=True)``
over a dataset whose ``__getitem__`` returns one pose, as one HIP launch per mini-batch (``dposer_batch_gather``, csrc/feed.hip).

The whole dataset sits in HBM (AMASS is a few million rows of 63 or 126 floats); the permutation of an epoch is computed per row inside
the kernel (rule: include/dposer_hip.h), never stored.  ``batch(step)`` is therefore a pure function of ``step``: a resumed run continues
on exactly the rows the uninterrupted run would have seen, and the ranks of a data-parallel job, which all use the SAME seed, read
disjoint slices of one global batch without exchanging anything.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import torch

from .. import _C
from .. import distributed as D


def feed_position(step, steps_per_epoch, batch_size, num_replicas=1, rank=0):
    """(epoch, base) of ``step``: the global batch of a step occupies positions [(step % steps_per_epoch) W B, + W B) of its epoch's
    permutation and rank r takes [r B, (r + 1) B) inside it."""
    epoch, within = divmod(int(step), int(steps_per_epoch))
    return epoch, (within * num_replicas + rank) * batch_size


def feed_steps_per_epoch(num_rows, batch_size, num_replicas=1):
    """N // (W B): drop_last, as run/train.py:79-84 -- the tail of each epoch's permutation is unused, as with a shuffling DataLoader.
    Fewer rows than one global batch is an error (the reference would spin forever in ``while step < num_train_steps``)."""
    if num_rows < num_replicas * batch_size:
        raise ValueError(f"{num_rows} rows do not fill one global batch of {num_replicas} x {batch_size}: with drop_last an epoch "
                         "would have no step")
    return num_rows // (num_replicas * batch_size)


class DeviceFeed:
    def __init__(self, poses, batch_size, *, seed=0, shapes=None, num_replicas=None, rank=None, device=None):
        self.num_replicas = D.world_size() if num_replicas is None else int(num_replicas)
        self.rank = D.rank() if rank is None else int(rank)
        if not 0 <= self.rank < self.num_replicas:
            raise ValueError(f"rank {self.rank} outside [0, {self.num_replicas})")
        self.batch_size = int(batch_size)
        if self.batch_size < 1:
            raise ValueError("batch_size must be >= 1")
        self._check_rows(poses, "poses")
        self.N, self.D = int(poses.shape[0]), int(poses.shape[1])
        if shapes is not None:
            self._check_rows(shapes, "shapes")
            if shapes.shape[0] < self.N:
                raise ValueError(f"shapes has {shapes.shape[0]} rows, fewer than the {self.N} poses")
        self.steps_per_epoch = feed_steps_per_epoch(self.N, self.batch_size, self.num_replicas)
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        if not torch.cuda.is_available():
            raise _C.DPoserHipError("DeviceFeed keeps the dataset in GPU memory and gathers with a HIP kernel: no GPU, no feed (no CPU fallback)")
        if device is None:
            device = poses.device if poses.is_cuda else torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        self.poses = poses.detach().to(self.device).contiguous()
        self.shapes = None if shapes is None else shapes.detach().to(self.device).contiguous()
        _C.require_gpu(self.poses, "DeviceFeed")

    @staticmethod
    def _check_rows(t, name):
        if not torch.is_tensor(t) or t.dim() != 2 or t.dtype != torch.float32 or t.shape[0] < 1 or t.shape[1] < 1:
            raise ValueError(f"{name} must be a non-empty 2-D float32 tensor")

    def __len__(self):
        return self.steps_per_epoch

    def epoch_of(self, step):
        return int(step) // self.steps_per_epoch

    def position(self, step):
        return feed_position(step, self.steps_per_epoch, self.batch_size, self.num_replicas, self.rank)

    def gather(self, epoch, base, count, *, out=None, aux_out=None, indices=None):
        """Rows pi(seed, epoch, base .. base + count) into the given device tensors (each optional): the raw call."""
        for name, t, dt, cols in (("out", out, torch.float32, self.D), ("aux_out", aux_out, torch.float32, None),
                                  ("indices", indices, torch.int64, None)):
            if t is None:
                continue
            _C.require_gpu(t, name)
            if t.dtype != dt or not t.is_contiguous():
                raise ValueError(f"{name} must be a contiguous {dt} tensor")
        if aux_out is not None and self.shapes is None:
            raise ValueError("aux_out given, but the feed holds no shapes")
        if out is not None and tuple(out.shape) != (count, self.D):
            raise ValueError(f"out must be [{count}, {self.D}]")
        if aux_out is not None and tuple(aux_out.shape) != (count, self.shapes.shape[1]):
            raise ValueError(f"aux_out must be [{count}, {self.shapes.shape[1]}]")
        if indices is not None and tuple(indices.shape) != (count,):
            raise ValueError(f"indices must be [{count}]")
        a = _C.BatchGatherArgs()
        a.data, a.N, a.D = self.poses.data_ptr(), self.N, self.D
        if self.shapes is not None:
            a.aux, a.N_aux, a.D_aux = self.shapes.data_ptr(), int(self.shapes.shape[0]), int(self.shapes.shape[1])
        a.base, a.B, a.seed, a.epoch = int(base), int(count), self.seed, int(epoch)
        a.out = None if out is None else out.data_ptr()
        a.aux_out = None if aux_out is None else aux_out.data_ptr()
        a.indices = None if indices is None else indices.data_ptr()
        with torch.cuda.device(self.device):
            _C.check(_C.lib().dposer_batch_gather(C.byref(a), _C.stream_ptr()), "dposer_batch_gather")

    def batch(self, step):
        """The mini-batch of ``step`` on this rank: [B, D], or {'poses', 'shapes'} when the feed holds shapes."""
        epoch, base = self.position(step)
        out = torch.empty(self.batch_size, self.D, dtype=torch.float32, device=self.device)
        if self.shapes is None:
            self.gather(epoch, base, self.batch_size, out=out)
            return out
        aux = torch.empty(self.batch_size, self.shapes.shape[1], dtype=torch.float32, device=self.device)
        self.gather(epoch, base, self.batch_size, out=out, aux_out=aux)
        return {"poses": out, "shapes": aux}

    def indices(self, step):
        """int64 [B]: the dataset rows ``batch(step)`` holds (the same kernel, index-only)."""
        epoch, base = self.position(step)
        idx = torch.empty(self.batch_size, dtype=torch.int64, device=self.device)
        self.gather(epoch, base, self.batch_size, indices=idx)
        return idx
