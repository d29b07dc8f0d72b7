"""Data parallelism for the finetune path: one process per GPU, full replica each, disjoint sample shards, and ONE
exchange step -- the gradient all-reduce -- exactly the reference's default ``DDPStrategy``
(videotuna/utils/train_utils.py:127-139, scripts/train.py:215-217).  Because every trainable tensor lives in one
flat fp32 buffer (vt355.lora.LoraState) the exchange is a single RCCL all-reduce (7.4 MB for CogVideoX-2B r=4),
issued asynchronously so the next micro-batch's input preparation overlaps it; the 1/world average is folded into
the fused AdamW's ``grad_scale`` (no extra pass over the gradients).  ``no_sync`` semantics: call ``reduce`` only on
the last micro-batch of an accumulation window.
"""
from __future__ import annotations

import os
from typing import Optional

import torch
import torch.distributed as dist


def init_from_env(backend: Optional[str] = None):
    """torchrun-style rendezvous (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_*).  Returns (rank, local_rank, world)."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1 and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29500")
        if backend is None:
            backend = "nccl" if torch.cuda.is_available() else "gloo"     # "nccl" is RCCL on ROCm
        if backend == "nccl":
            torch.cuda.set_device(local)
        dist.init_process_group(backend=backend, rank=rank, world_size=world)
    return rank, local, world


def sync_chain_guard(like: torch.Tensor, group=None):
    """All ranks agree on the attention backward's sticky time-out word before the optimizer reads it: the MAX over the group is written
    back into every rank's word (ops.chain_guard), so vt_adamw's guard refuses the update on EVERY rank and FusedAdamW.check_errors raises
    on all of them at the next step -- a rank that alone skipped its update would leave the replicas diverged and the others waiting in
    the next collective.  One 4-byte all-reduce per step; nothing to do for CPU tensors (gloo rehearsals) or a single rank."""
    if not (dist.is_initialized() and dist.get_world_size(group) > 1) or like.device.type != "cuda":
        return
    from . import ops
    guard = ops.chain_guard(like.device)
    flag = guard.clone() if guard is not None else torch.zeros(1, dtype=torch.int32, device=like.device)
    dist.all_reduce(flag, op=dist.ReduceOp.MAX, group=group)
    if guard is not None:
        guard.copy_(flag)


class FlatGradReducer:
    """All-reduce (sum) of a flat gradient buffer; ``grad_scale`` = 1/world turns the sum into the DDP mean.

    Gradient clipping needs no communication of its own, but it needs this ORDER: ``reduce()`` (or ``reduce_async()`` + ``wait()``)
    first, then ``optimizer.step(grad_scale=reducer.grad_scale)``.  The optimizer's norm pass then reads the SUMMED gradient, identical
    on every rank, and ``grad_scale * |sum|`` is the norm of the mean gradient that Lightning's DDP clips; every rank derives the same
    coefficient, bit for bit (the norm kernels use no atomics).  A step issued before ``wait()`` would clip a partial sum."""

    def __init__(self, flat_grad: torch.Tensor, group=None):
        self.grad = flat_grad
        self.group = group
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self._work = None

    @property
    def grad_scale(self) -> float:
        return 1.0 / self.world

    def reduce_async(self):
        if self.world > 1:
            self._work = dist.all_reduce(self.grad, op=dist.ReduceOp.SUM, group=self.group, async_op=True)

    def wait(self):
        if self._work is not None:
            self._work.wait()
            self._work = None
            sync_chain_guard(self.grad, self.group)

    def reduce(self):
        self.reduce_async()
        self.wait()


def shard_indices(n_items: int, rank: int, world: int):
    """DistributedSampler-style disjoint shard (no shuffling): item i goes to rank i % world."""
    return list(range(rank, n_items, world))


def broadcast_flat(flat: torch.Tensor, src: int = 0, group=None):
    if dist.is_initialized() and dist.get_world_size(group) > 1:
        dist.broadcast(flat, src=src, group=group)


class BucketedReducer:
    """Full fine-tuning: the flat fp32 gradient buffer (6.8 GB for CogVideoX-2B) is all-reduced in slices as the backward
    finishes them -- one slice per transformer block, last block first, ~225 MB each -- with ``async_op=True`` so RCCL
    runs them on its own stream while the engine keeps computing earlier blocks (the DDP bucket overlap of the reference's
    ``DDPStrategy``, without re-bucketing copies: the slices ARE the gradient storage).  xGMI is point-to-point: a few
    large slices keep every link busy; the 1/world mean is folded into the optimizer's ``grad_scale``.
    Install ``reducer.hook`` as ``FullFTState.on_grads_ready`` for the LAST micro-batch of an accumulation window only
    (``no_sync`` semantics), then ``wait_all()`` before the optimizer step.  With gradient clipping that order is a requirement of
    correctness, not only of completeness: the optimizer's norm pass must read the fully summed buffer (see FlatGradReducer)."""

    def __init__(self, flat_grad: torch.Tensor, group=None, wire_dtype: Optional[torch.dtype] = None):
        """wire_dtype torch.bfloat16: every slice travels as bf16 (3.4 GB instead of 6.8 GB per step for CogVideoX-2B -- SURVEY 8(e)'s
        budget, and what the reference's DDP moves: its gradients ARE bf16); the fp32 buffer receives the reduced values back.
        None: the fp32 slices themselves are reduced in place (bit-stable sums, twice the bytes)."""
        self.grad = flat_grad
        self.group = group
        self.wire_dtype = wire_dtype
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self._works = []
        self.covered = 0
        self.bytes_sent = 0

    @property
    def grad_scale(self) -> float:
        return 1.0 / self.world

    def hook(self, lo: int, hi: int):
        self.covered += hi - lo
        if self.world > 1:
            if self.wire_dtype is None:
                buf = None
                work = dist.all_reduce(self.grad[lo:hi], op=dist.ReduceOp.SUM, group=self.group, async_op=True)
                self.bytes_sent += (hi - lo) * self.grad.element_size()
            else:
                buf = self.grad[lo:hi].to(self.wire_dtype)
                work = dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=self.group, async_op=True)
                self.bytes_sent += (hi - lo) * buf.element_size()
            self._works.append((work, lo, hi, buf))

    def wait_all(self):
        for w, lo, hi, buf in self._works:
            w.wait()
            if buf is not None:
                self.grad[lo:hi].copy_(buf)
        if self._works:
            sync_chain_guard(self.grad, self.group)
        self._works = []
        covered, self.covered = self.covered, 0
        return covered
