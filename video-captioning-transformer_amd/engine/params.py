"""The parameter set of one model (fp32 masters, gradients, compute-dtype shadow, transposed / packed weight copies, Adam tables)
and the named static buffers the engines work in."""
import bisect
from dataclasses import dataclass
from typing import Dict, List, Optional

import torch

from .. import ops


# The derived weight copies a step keeps in sync with the compute-dtype shadow.  Plain records: ParamSet's methods hold the behaviour.

@dataclass(eq=False, slots=True)
class TransposedCopy:
    """A [cols, ld] transposed copy of one weight matrix (ParamSet.transposed[name])."""
    t: torch.Tensor
    start: int          # flat elements [start, end) of the weight
    end: int
    eager: bool         # rewritten whenever the shadow of the weight is; else on demand (want_transposed)
    version: int        # ParamSet.version the copy was made at (-1: never written)


@dataclass(eq=False, slots=True)
class PackedPart:
    """One part (a layer, or the unify weight in front of an encoder stack) of a packed stream."""
    start: int          # flat elements [start, end) that hold the part's weights
    end: int
    blocks: list        # (2-D shadow view, nchunks, first chunk in the stream[, transposed]): what ops.ss_pack takes
    dirty: bool         # the shadow moved on and nobody re-packed the part yet


@dataclass(eq=False, slots=True)
class PackedStream:
    """The weights of a whole stack in the order the sample-stationary kernel consumes them (ParamSet.packed[key])."""
    t: torch.Tensor
    firsts: list        # first chunk of every part
    parts: List[PackedPart]


@dataclass(eq=False, slots=True)
class AdamPackSeg:
    """One weight whose packed copy the optimizer's pass writes itself (a row of the device table of vct_adam_pack_seg)."""
    begin: int          # flat elements [begin, end) of the weight
    end: int
    K: int
    mode: int           # 0: blocks of 512 rows, 1: slices of 512 columns
    chunk0: list        # first chunk of each of the (up to) 4 blocks, -1: not packed
    stream: int         # device pointer of the packed stream


@dataclass(eq=False, slots=True)
class AdamPackEntry:
    """What ParamSet.adam_pack_table caches per (range, set of streams)."""
    table: Optional[torch.Tensor]
    nseg: int
    parts: List[PackedPart]
    segs: Dict[str, AdamPackSeg]


class StepContext:
    """Per-model execution state shared by the engines of ONE parameter set: the side HIP stream (+ its split-K scratch) that
    weight-gradient GEMMs / the encoder backward / the decoder prefix run on, and the buffer generation counter that
    invalidates baked pointer sets (launch lists, hipGraphs, pointer tables).  It used to be process-global: two models in one
    process (a training model and an evaluation copy) then shared a side stream and dropped each other's recordings."""

    def __init__(self):
        self.side = None
        self.side_ws = None
        self.generation = 0


class ParamSet:
    """fp32 master parameters (views of one flat buffer), their fp32 gradient views and the
    compute-dtype shadow used by the GEMMs.  Order = gradient-ready order of the backward pass so
    that contiguous slices of the flat gradient buffer are the all-reduce buckets."""

    ALIGN = 64  # elements; keeps every view 16-byte aligned in fp32 and bf16

    def __init__(self, named: List, device, compute_dtype: torch.dtype, no_shadow=()):
        self.names = [n for n, _ in named]
        self.params = {n: p for n, p in named}
        self.device, self.compute_dtype = device, compute_dtype
        self.ctx = StepContext()
        self.offsets, off = {}, 0
        for n, p in named:
            self.offsets[n] = off
            off += (p.numel() + self.ALIGN - 1) // self.ALIGN * self.ALIGN
        self.total = off
        self.flat = torch.zeros(self.total, dtype=torch.float32, device=device)
        self.gflat = torch.zeros(self.total, dtype=torch.float32, device=device)
        self.no_shadow = set(no_shadow)
        for n, p in named:
            o, k = self.offsets[n], p.numel()
            view = self.flat[o:o + k].view(p.shape)
            view.copy_(p.data.to(device=device, dtype=torch.float32))
            p.data = view
        self.g = {n: self.gflat[self.offsets[n]:self.offsets[n] + p.numel()].view(p.shape) for n, p in named}
        if compute_dtype == torch.float32:
            self.cflat = self.flat
            self.c = {n: p.data for n, p in named}
        else:
            self.cflat = torch.zeros(self.total, dtype=compute_dtype, device=device)
            self.c = {n: self.cflat[self.offsets[n]:self.offsets[n] + p.numel()].view(p.shape) for n, p in named}
        self._stamp = None
        self.version = 0        # bumped whenever the shadow is (or may have been) rewritten: lazy transposed copies key on it
        # transposed copies of individual weight matrices in the compute dtype (name -> TransposedCopy): kept in
        # step with the shadow by refresh_shadow / cast_range / FusedAdam.step_range (refresh_transposed)
        self.transposed: Dict[str, TransposedCopy] = {}
        # STREAM-ORDER packed copies of whole stacks (key -> PackedStream): the operand of the
        # sample-stationary layer kernels (ops.layer_ss_fwd), kept in step with the shadow exactly like the eager transposed copies
        self.packed: Dict[str, PackedStream] = {}
        self._adam_pack: Dict[tuple, AdamPackEntry] = {}
        # the optimizer that steps weight matrices INSIDE their weight-gradient GEMMs (trainer.FusedAdam.enable_dw_fusion; None: nobody
        # does): _StackBase.dw_gemm asks it for the epilogue descriptor of every gradient view it is about to produce
        self.dw_adam = None
        # False after a step whose weight-gradient GEMMs consumed their gradients in registers (optimizer epilogue, store_grad = 0): the
        # 2-D weights' regions of gflat (and their .grad views) then hold values of an EARLIER backward.  MMT4Caption.grads_valid.
        self.weight_grads_valid = True
        self._starts = None
        # contiguous [start, end) ranges to cast (everything except the no_shadow tensors)
        self.cast_ranges, start = [], 0
        for n in self.names:
            if n in self.no_shadow:
                if self.offsets[n] > start:
                    self.cast_ranges.append((start, self.offsets[n]))
                start = self.offsets[n] + (self.params[n].numel() + self.ALIGN - 1) // self.ALIGN * self.ALIGN
        if start < self.total:
            self.cast_ranges.append((start, self.total))

    def intact(self) -> bool:
        """True while every nn.Parameter still aliases the flat buffer (Module.to() would break it)."""
        base = self.flat.data_ptr()
        for n in (self.names[0], self.names[-1]):
            if self.params[n].data_ptr() != base + 4 * self.offsets[n]:
                return False
        return True

    def _masters_stamp(self) -> int:
        return sum(p._version for p in self.params.values())

    @property
    def stamp(self):
        """Changes whenever the masters were written since the shadow last followed them (None: never cast)."""
        return self._stamp

    def refresh_shadow(self, force=False):
        """bf16 shadow <- fp32 masters (one cast kernel per contiguous range)."""
        if self.compute_dtype == torch.float32:
            return
        stamp = None
        if not force:
            stamp = self._masters_stamp()
            if stamp == self._stamp:
                return
        for a, b in self.cast_ranges:
            ops.cast(self.flat[a:b], self.cflat[a:b])
        self.version += 1
        self.refresh_transposed(0, self.total)
        self._stamp = stamp if stamp is not None else self._masters_stamp()

    def masters_written(self):
        """A torch optimizer wrote the fp32 masters: re-cast the shadow and take the new stamp (fp32 mode: the stamp only)."""
        self.refresh_shadow(force=True)
        self._stamp = self._masters_stamp()

    def optimizer_stepped(self):
        """The fused optimizer stepped the masters and rewrote the shadow (and the eager copies) itself."""
        self.version += 1
        self._stamp = self._masters_stamp()

    def shadow_replayed(self):
        """A replayed recording of a step rewrote the shadow (lazy transposed copies key on `version`)."""
        self.version += 1

    def cast_range(self, a: int, b: int):
        """bf16 shadow <- fp32 masters for flat elements [a, b) (minus the tensors that have no shadow)."""
        if self.compute_dtype == torch.float32:
            return
        for x, y in self.cast_ranges:
            lo, hi = max(a, x), min(b, y)
            if hi > lo:
                ops.cast(self.flat[lo:hi], self.cflat[lo:hi])
        self.version += 1
        self.refresh_transposed(a, b)

    def want_transposed(self, name: str, eager: bool = False) -> torch.Tensor:
        """A [cols, ld >= rows] transposed copy (compute dtype) of the 2-D weight `name`, created on first use.
        eager=True (a training-step operand: W_g^T of the NT-form vocabulary dX): rewritten whenever the shadow of that weight
        is -- by the optimizer's own pass when it is FusedAdam (vct_adam_step_2d), else by a transpose launch behind it.
        eager=False (decode-time operands): refreshed HERE, on demand, when the shadow has changed since the copy was made
        (`version` counts shadow rewrites): a training loop that validates between epochs pays nothing per step for them."""
        ent = self.transposed.get(name)
        if ent is None:
            w = self.c[name]
            rows, cols = w.shape
            t = torch.zeros(cols, (rows + 31) // 32 * 32, dtype=w.dtype, device=w.device)
            a = self.offsets[name]
            ent = self.transposed[name] = TransposedCopy(t, a, a + w.numel(), bool(eager), -1)
        was_lazy = not ent.eager
        if eager:
            ent.eager = True
        if ent.version != self.version:
            if ent.version < 0 or was_lazy:           # new, or a (so far) lazy copy that is out of date
                ops.transpose(self.c[name], ent.t)
            ent.version = self.version
        return ent.t

    def want_packed(self, key: str, layers):
        """(stream, [first chunk of every part]): the weights of a whole Transformer STACK packed, part after part, in the order the
        sample-stationary kernel consumes them (include/vct_hip.h, vct_ss_pack).  layers = [(names, blocks_fn)] per part (a layer, or
        the unify weight in front of an encoder stack), blocks_fn() -> [(2-D shadow view, nchunks, first chunk inside the part)].
        Created on first use; every part is rewritten whenever the shadow of its weights is (refresh_transposed: behind the
        optimizer's pass, inside the recorded step)."""
        ent = self.packed.get(key)
        if ent is None:
            parts, at, firsts = [], 0, []
            for names, blocks_fn in layers:
                blocks = blocks_fn()                        # (w, nchunks, first chunk[, transposed])
                n = max(blk[2] + blk[1] for blk in blocks)
                parts.append((names, [(blk[0], blk[1], blk[2] + at) + tuple(blk[3:]) for blk in blocks]))
                firsts.append(at)
                at += n
            t = torch.empty(at * ops.SS_CHUNK, dtype=self.compute_dtype, device=self.device)
            subs = []
            for names, blocks in parts:
                a = min(self.offsets[n] for n in names)
                b = max(self.offsets[n] + self.params[n].numel() for n in names)
                subs.append(PackedPart(a, b, blocks, True))
            ent = self.packed[key] = PackedStream(t, firsts, subs)
            # a NEW stream changes what a step launches (the optimizer's pass / the pack launch behind it now also writes this
            # stream): recordings made before it existed would replay without refreshing it -> drop them (ctx.generation is what
            # CaptionTrainer keys its launch lists / graphs on)
            self.ctx.generation += 1
        todo = []
        for part in ent.parts:
            if part.dirty:
                todo += part.blocks
                part.dirty = False
        if todo:
            ops.ss_pack(todo, ent.t)
        return ent.t, ent.firsts

    def refresh_lazy_transposed(self):
        """Bring every on-demand transposed copy up to date (decode entry points call this before replaying captured steps,
        which bake the copies' addresses but cannot notice that the weights moved on)."""
        for name, ent in self.transposed.items():
            if not ent.eager and ent.version != self.version:
                ops.transpose(self.c[name], ent.t)
                ent.version = self.version

    def name_at(self, off: int):
        """(parameter name, its first flat element) of the parameter that holds flat element `off`."""
        if self._starts is None:
            self._starts = sorted((o, n) for n, o in self.offsets.items())
        i = bisect.bisect_right(self._starts, (off, chr(0x10ffff))) - 1
        return self._starts[i][1], self._starts[i][0]

    def pack_seg(self, name: str):
        """The AdamPackSeg of the stream-order packed copy the optimizer can maintain for the weight `name` (adam_pack_table's
        eligibility rules), or None."""
        return self._adam_pack_entry(0, self.total).segs.get(name)

    def adam_pack_table(self, a: int, b: int):
        """(device table of vct_adam_pack_seg, entries, [parts]) for the packed parts whose weights lie inside flat elements [a, b):
        the optimizer's pass over [a, b) writes their stream-order copies itself (ops.adam_step(pack=...)).  Parts with transposed
        blocks (the backward's stream) and matrices whose blocks are not whole 512-row blocks / 512-column slices stay with vct_ss_pack.
        The table is built once per (a, b) and set of streams (pointers are static)."""
        hit = self._adam_pack_entry(a, b)
        return hit.table, hit.nseg, hit.parts

    def _adam_pack_entry(self, a: int, b: int) -> AdamPackEntry:
        key = (a, b, tuple(sorted(self.packed)))
        hit = self._adam_pack.get(key)
        if hit is not None:
            return hit
        starts = sorted((off, n) for n, off in self.offsets.items())
        segs, parts = {}, []
        c0 = self.cflat.data_ptr()
        # ONE choice of stream per weight for the whole parameter set: the table of a sub-range is the whole-buffer selection
        # filtered to [a, b) -- the GEMM epilogues take their packed-stream targets from the (0, total) table (pack_seg) and step_range
        # marks parts as written from the (a, b) one; built independently the two could settle on different streams for a weight
        # that two eligible streams hold, and the one nobody writes would go stale
        full = None
        if (a, b) != (0, self.total):
            full = set(id(x) for x in self._adam_pack_entry(0, self.total).parts)
        for ent in self.packed.values():
            for sub in ent.parts:
                if not (a <= sub.start and sub.end <= b):
                    continue
                if full is not None and id(sub) not in full:
                    continue
                ok, mine = True, {}
                for blk in sub.blocks:
                    w, nch, dc = blk[:3]
                    if len(blk) > 3 and blk[3]:
                        ok = False
                        break
                    eo = (w.data_ptr() - c0) // 2
                    i = bisect.bisect_right(starts, (eo, chr(0x10ffff))) - 1
                    mo, name = starts[i]
                    shape = self.params[name].shape
                    if len(shape) != 2 or w.stride(0) != shape[1]:
                        ok = False
                        break
                    N, K = shape
                    r0, cc0 = (eo - mo) // K, (eo - mo) % K
                    if cc0 == 0 and nch * 64 == K and r0 % 512 == 0 and r0 // 512 < 4:
                        mode, idx = 0, r0 // 512
                    elif r0 == 0 and N == 512 and nch == 8 and cc0 % 512 == 0 and cc0 // 512 < 4:
                        mode, idx = 1, cc0 // 512
                    else:
                        ok = False
                        break
                    if dc >= 0xffff:
                        ok = False            # the kernels carry the first chunk of a block as a 16-bit field (0xffff = "not packed"): a
                        break                 # stream of >= 4 GiB stays with vct_ss_pack instead of silently going stale
                    if name in segs and segs[name].stream != ent.t.data_ptr():
                        ok = False            # another stream already holds this weight: the kernel's table has ONE stream per weight,
                        break                 # so this part stays with vct_ss_pack (refresh_transposed) instead of going stale
                    sg = mine.get(name)
                    if sg is None:
                        sg = mine[name] = AdamPackSeg(mo, mo + N * K, K, mode, [-1, -1, -1, -1], ent.t.data_ptr())
                    if sg.mode != mode:
                        ok = False
                        break
                    sg.chunk0[idx] = dc
                if ok and mine:
                    segs.update(mine)
                    parts.append(sub)
        rows = sorted(segs.values(), key=lambda sg: sg.begin)      # (one segment per weight: the begins are distinct)
        if rows:
            arr = (ops.L.AdamPackSeg * len(rows))()
            for i, sg in enumerate(rows):
                arr[i].begin, arr[i].end, arr[i].K, arr[i].mode, arr[i].stream = sg.begin, sg.end, sg.K, sg.mode, sg.stream
                for j in range(4):
                    arr[i].chunk0[j] = sg.chunk0[j]
            raw = bytes(arr)
            table = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(self.device)
        else:
            table = None
        hit = self._adam_pack[key] = AdamPackEntry(table, len(rows), parts, segs)
        return hit

    def refresh_transposed(self, a: int, b: int, skip=(), packed_done=()):
        """Shadow elements [a, b) were just rewritten: eager transposed copies inside follow (except `skip`: already written by
        the optimizer's fused pass); lazy ones are picked up by want_transposed through `version`.  packed_done: parts of packed
        streams the optimizer's pass wrote itself (adam_pack_table)."""
        for name, ent in self.transposed.items():
            if ent.eager and name not in skip and a <= ent.start and ent.end <= b:
                ops.transpose(self.c[name], ent.t)
        done = set(id(x) for x in packed_done)
        for ent in self.packed.values():
            todo = []
            for sub in ent.parts:
                if id(sub) in done:
                    sub.dirty = False
                    continue
                if sub.end > a and sub.start < b:             # the rewritten range touches this part
                    if a <= sub.start and sub.end <= b:
                        todo += sub.blocks
                        sub.dirty = False
                    else:                                     # partly rewritten (no schedule does this): re-pack at the next use
                        sub.dirty = True
            if todo:
                ops.ss_pack(todo, ent.t)                      # every part of the stack this pass rewrote: one launch (<= 48 blocks)

    def eager_transposed_in(self, a: int, b: int):
        """[(name, tensor, start, end)] of the eager transposed copies whose weight lies inside flat elements [a, b)."""
        return [(n, e.t, e.start, e.end) for n, e in self.transposed.items() if e.eager and a <= e.start and e.end <= b]

    def install_grads(self):
        for n, p in self.params.items():
            if p.requires_grad and p.grad is not self.g[n]:
                if p.grad is not None and p.grad.data_ptr() != self.g[n].data_ptr():
                    self.g[n].add_(p.grad)  # honour a pre-existing accumulated gradient
                p.grad = self.g[n]


class _Buf:
    """Named device buffers with STATIC addresses.  One instance serves every shape configuration of an engine:
    `get` hands out a leading view of a per-name allocation that only ever grows, so a ragged epoch (the loader trims S
    to each batch's longest caption) neither re-allocates per step nor frees memory that a captured hipGraph / recorded
    launch list still points to.  `ctx.generation` (StepContext of the owning parameter set) counts (re)allocations: whoever
    bakes pointers (trainer graphs, launch lists, pointer tables) keys its cache on it and re-records after a growth."""

    def __init__(self, device, ctx: "StepContext"):
        self.device, self.t, self._store, self.ctx = device, {}, {}, ctx

    def get(self, name, shape, dtype):
        n = 1
        for s in shape:
            n *= int(s)
        st = self._store.get(name)
        if st is None or st.dtype != dtype or st.numel() < n:
            st = torch.empty(max(n, 1), dtype=dtype, device=self.device)
            self._store[name] = st
            self.ctx.generation += 1
            for k in [k for k in self.t if isinstance(k, tuple) and k and k[0] == "ln_table"]:
                del self.t[k]          # pointer tables baked the old addresses
        t = st[:n].view(shape)
        self.t[name] = t
        return t

