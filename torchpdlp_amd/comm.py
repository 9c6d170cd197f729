"""Comm: the collectives of a sharded problem over ``torch.distributed`` (backend ``nccl`` = RCCL over xGMI; ``gloo`` in the
tests and rehearsals that put several ranks on one card).  It knows the process group and nothing of an engine."""
from __future__ import annotations

import torch


class Comm:
    """One process per GPU.  Vectors are sharded in equal blocks (the LP is padded so the sizes divide)."""

    def __init__(self, group=None, dist=None):
        if dist is None:
            import torch.distributed as dist
        self.dist = dist
        self.group = group
        self.rank = dist.get_rank(group)
        self.world = dist.get_world_size(group)
        self.backend = dist.get_backend(group)

    def _detour(self, t: torch.Tensor) -> bool:
        """gloo has no device collectives (test path): such a tensor travels through the host, synchronously"""
        return self.backend == "gloo" and t.is_cuda

    def _via_host(self, t: torch.Tensor, collective, load: bool = True):
        """the detour: a host tensor like ``t`` (a copy of it with ``load``), the collective on that, the result back into ``t``"""
        host = t.cpu() if load else torch.empty(t.numel(), dtype=t.dtype)
        collective(host)
        t.copy_(host)

    def coll_device(self, device):
        """where a small tensor that travels over the group has to live: the host under gloo, ``device`` otherwise"""
        return "cpu" if self.backend == "gloo" or device is None else device

    def agree(self, ok, device=None) -> int:
        """MIN over the ranks of a flag: did EVERY rank succeed?  (the flag lives where ``coll_device`` says)"""
        flag = torch.tensor([int(bool(ok))], dtype=torch.int32, device=self.coll_device(device))
        self.dist.all_reduce(flag, op=self.dist.ReduceOp.MIN, group=self.group)
        return int(flag)

    def all_gather(self, full: torch.Tensor, async_op: bool = False):
        """full = concat over ranks of equal shards; this rank's shard is already in place.  ``async_op``: not waited for --
        returns a handle whose ``wait()`` makes the current stream wait (None: already done)"""
        shard = full.numel() // self.world
        mine = full[self.rank * shard:(self.rank + 1) * shard]
        if self._detour(full):
            return self._via_host(full, lambda host: self.dist.all_gather_into_tensor(host, mine.cpu(), group=self.group), load=False)
        return self.dist.all_gather_into_tensor(full, mine, group=self.group, async_op=async_op)

    def all_gather_async(self, full: torch.Tensor):
        return self.all_gather(full, async_op=True)

    def all_gather_piece(self, full: torch.Tensor, lo: int, hi: int):
        """elements [lo, hi) of EVERY rank's block of ``full`` (this rank's are in place); returns a handle whose ``wait()`` makes the
        current stream wait for the piece (None: already there) -- the pieces of a chunked exchange queue up behind each other while
        the products of the earlier ones run"""
        B = full.numel() // self.world
        views = [full[q * B + lo:q * B + hi] for q in range(self.world)]
        if hi <= lo:
            return None
        if self._detour(full):      # (its own detour: only the OTHER ranks' pieces come back from the host)
            parts = [torch.empty(hi - lo, dtype=full.dtype) for _ in range(self.world)]
            self.dist.all_gather(parts, views[self.rank].cpu(), group=self.group)
            for q, part in enumerate(parts):
                if q != self.rank:
                    views[q].copy_(part)
            return None
        # (the input is a copy of this rank's piece: an output list that aliases the input is not something to try for the first
        # time inside a timed run; the copy is 1/world of a piece)
        return self.dist.all_gather(views, views[self.rank].clone(), group=self.group, async_op=True)

    def all_reduce(self, t: torch.Tensor, op):
        reduce = lambda v: self.dist.all_reduce(v, op=op, group=self.group)
        if self._detour(t):
            self._via_host(t, reduce)
        else:
            reduce(t)

    def all_reduce_sum(self, t: torch.Tensor, op=None):
        self.all_reduce(t, self.dist.ReduceOp.SUM if op is None else op)

    def all_reduce_max(self, t: torch.Tensor):
        self.all_reduce(t, self.dist.ReduceOp.MAX)

    def all_reduce_min(self, t: torch.Tensor):
        self.all_reduce(t, self.dist.ReduceOp.MIN)

    def all_reduce_sum_async(self, t: torch.Tensor):
        """the same reduction, not waited for: returns a handle whose ``wait()`` makes the current stream wait (None: already done)"""
        if self._detour(t):
            self.all_reduce_sum(t)
            return None
        return self.dist.all_reduce(t, op=self.dist.ReduceOp.SUM, group=self.group, async_op=True)
