"""The two gradient exchanges of the data-parallel step: all-reduce of the gradient buckets (GradExchange, any optimizer) and
reduce-scatter -> Adam on the owned shard -> all-gather (ShardedExchange, the fused optimizer)."""
import contextlib
from typing import List, Optional

import torch
import torch.distributed as dist

from .. import ops


class GradExchange:
    """Gradient averaging across data-parallel ranks (one process per GPU).

    * init: rank 0's parameters (the flat fp32 buffer) are broadcast, like DDP's constructor.
    * per step: for each bucket of MMT4Caption.grad_buckets() an async all-reduce(SUM) is issued on
      the communication stream the backend owns, ordered after the kernels already enqueued on the
      compute stream; `finish()` makes the compute stream wait for them and applies 1/world.
    * payload: fp32 by default; `payload_dtype=torch.bfloat16` halves the xGMI bytes (cast kernels
      from libvct_hip.so on both sides)."""

    def __init__(self, model, group=None, payload_dtype: Optional[torch.dtype] = None, broadcast: bool = True,
                 force: bool = False):
        self.model, self.group = model, group
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.active = self.world > 1 or (force and dist.is_initialized())   # force: run the collectives even alone
        self.buckets = model.grad_buckets()
        self.payload_dtype = payload_dtype
        self._work: List = []
        self._stage = None
        self._avg = dist.is_initialized() and dist.get_backend(group) == "nccl"   # RCCL has ReduceOp.AVG; gloo does not
        if payload_dtype is not None and payload_dtype != torch.float32:
            self._stage = torch.empty(model.flat_grads.numel(), dtype=payload_dtype, device=model.flat_grads.device)
        if broadcast and self.active:
            dist.broadcast(model.flat_params, src=0, group=group)
            model._ps.refresh_shadow(force=True)

    def bucket_ready(self, i: int):
        if not self.active:
            return
        a, b = self.buckets[i]
        if b <= a:
            return
        g = self.model.flat_grads[a:b]
        if self._stage is not None and g.is_cuda:
            s = self._stage[a:b]
            ops.cast(g, s)
            g = s
        op = dist.ReduceOp.AVG if self._avg else dist.ReduceOp.SUM
        if g.is_cuda and not self._avg:
            # gloo carrying CUDA buffers (several ranks sharing one GPU in the tests): its staging copy runs on a pool stream
            # behind an event of the current stream; seen once in a while with 4 ranks time-slicing one GPU: a rank's bucket read
            # before its producers had finished.  The host waits for the stream here (test path only; RCCL is stream-ordered
            # through the library's own event edges and never takes this branch)
            torch.cuda.current_stream().synchronize()
        self._work.append((dist.all_reduce(g, op=op, group=self.group, async_op=True), i))

    def finish(self, on_bucket_done=None):
        """Wait for every bucket's reduction (in issue order).  on_bucket_done(a, b) runs right after bucket
        [a, b) holds the averaged gradient -- the trainer uses it to start Adam on that range while later
        buckets are still on the wire."""
        if not self.active:
            return
        for w, i in self._work:
            w.wait()
            a, b = self.buckets[i]
            if self._stage is not None and self.model.flat_grads.is_cuda:
                ops.cast(self._stage[a:b], self.model.flat_grads[a:b])
            if not self._avg:
                self.model.flat_grads[a:b].mul_(1.0 / self.world)
            if on_bucket_done is not None:
                on_bucket_done(a, b)
        self._work.clear()


class ShardedExchange:
    """Gradient exchange + optimizer of the data-parallel step with the optimizer SHARDED over the ranks (ZeRO-1 style):

        per gradient bucket [a, b), as soon as backward has enqueued its last kernel (n = (b - a) / W, r = own rank):
            reduce-scatter(AVG)  g[a + r n : a + (r+1) n)  <- mean over ranks          (xGMI: (b-a)/W per link)
            Adam                 on that owned shard only                                (1/W of the 1.39 GB optimizer pass)
            all-gather           p[a:b) fp32 masters <- every rank's updated shard       (xGMI: (b-a)/W per link)
            cast                 bf16 shadow of [a:b) from the gathered masters          (local HBM: cheaper than shipping it)
        all of it on the communicator's own stream (coll.owns_stream), behind an event edge to the compute stream, so the
        wire and the optimizer run beside the rest of backward; finish() joins and bumps the Adam step counter.

    Against a plain all-reduce + replicated Adam the wire carries the same bytes (RS + AG = all-reduce) and the
    optimizer's HBM traffic drops by (W-1)/W.  payload_dtype=torch.bfloat16 halves the reduce-scatter bytes (gradients
    are rounded to bf16 before the mean; the all-gather stays fp32 so every rank holds identical masters).
    sharded=False (or a bucket that does not divide by W): all-reduce + Adam on the whole bucket.

    replaces: DistributedDataParallel's reducer + the replicated torch.optim.Adam (reference train.py:24-26, 217-219)."""

    def __init__(self, model, opt: "FusedAdam", coll, sharded: bool = True, payload_dtype: Optional[torch.dtype] = None,
                 broadcast: bool = True):
        self.model, self.opt, self.coll = model, opt, coll
        self.world, self.rank = coll.world, coll.rank
        self.active = True
        self.sharded = sharded
        self.buckets = model.grad_buckets()
        self.payload_dtype = payload_dtype if payload_dtype not in (None, torch.float32) else None
        self._stage = (torch.empty(model.flat_grads.numel(), dtype=self.payload_dtype, device=model.flat_grads.device)
                       if self.payload_dtype is not None else None)
        if broadcast and self.world > 1:
            coll.broadcast(model.flat_params, 0)
            coll.wait()
            model._ps.refresh_shadow(force=True)
        # each rank steps exp_avg / exp_avg_sq on its own shards only: the optimizer's state_dict() (checkpoints) must see
        # the gathered moments, so it calls back here first -- on every rank, it is a collective
        if self.sharded and self.world > 1:
            opt.pre_state_dict = self.gather_optimizer_state

    def _on_comm(self):
        return torch.cuda.stream(self.coll.stream) if self.coll.owns_stream else contextlib.nullcontext()

    def shard_of(self, i: int):
        a, b = self.buckets[i]
        W = self.world
        if not self.sharded or (b - a) % (8 * W) != 0:
            return None
        n = (b - a) // W
        return a + self.rank * n, a + (self.rank + 1) * n, n

    def bucket_ready(self, i: int):
        a, b = self.buckets[i]
        if b <= a:
            return
        m, coll = self.model, self.coll
        g, p = m.flat_grads, m.flat_params
        sh = self.shard_of(i)
        cur = torch.cuda.current_stream() if g.is_cuda else None
        if coll.owns_stream:
            ops.stream_wait(coll.stream, cur)          # the communicator's stream follows everything enqueued so far
        with self._on_comm():
            tag = f"comm_b{i}" if i < 8 else None          # live timing bracket of this bucket on the communicator's stream
            if tag:
                ops.tap(tag, 0)
            src = g
            if self._stage is not None:
                ops.cast(g[a:b], self._stage[a:b])
                src = self._stage
            if sh is None:
                coll.allreduce_avg(src[a:b], after=False)
                if src is not g:
                    ops.cast(src[a:b], g[a:b])
                self.opt.step_range(a, b)
                if tag:
                    ops.tap(tag, 1)
                return
            lo, hi, n = sh
            coll.reduce_scatter_avg(src[a:b], n, after=False)
            if src is not g:
                ops.cast(src[lo:hi], g[lo:hi])
            self.opt.step_range(lo, hi)
            coll.all_gather(p[a:b], n, after=False)
            m._ps.cast_range(a, b)
            if tag:
                ops.tap(tag, 1)

    def finish(self):
        ops.tap("comm_wait", 0)                  # compute stream: from "backward enqueued" to "the communicator's stream has drained"
        self.coll.wait()
        ops.tap("comm_wait", 1)
        self.opt.finish_ranges()

    def gather_optimizer_state(self):
        """Every rank's Adam moments are only current on its own shards: all-gather them (before a checkpoint)."""
        for i, (a, b) in enumerate(self.buckets):
            sh = self.shard_of(i)
            if sh is None or b <= a:
                continue
            for t in (self.opt.exp_avg, self.opt.exp_avg_sq):
                self.coll.all_gather(t[a:b], sh[2])
        self.coll.wait()

