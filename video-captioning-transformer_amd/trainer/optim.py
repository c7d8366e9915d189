"""The optimizer of the caption task: FusedAdam (one kernel over the flat parameter buffer, or the epilogues of the weight-gradient
GEMMs) and the reference's optimizer / scheduler factory."""
import os

import torch

from .. import ops
from .clip import KEYS as CLIP_KEYS, check_clip_settings


def owned_range(model, task):
    """[begin, end) of the flat parameter buffer the optimizer of `task` owns -- what the reference's filter(requires_grad) after
    mode(task) keeps (train.py:24): 'caption' (or None) the decoder and the encoder, 'match' the encoder and matching.* (the decoder
    is frozen), 'cross' everything."""
    if task in (None, "caption"):
        return 0, model.caption_param_end
    if task == "match":
        return model.encoder_param_begin, model._ps.total
    if task == "cross":
        return 0, model._ps.total
    raise ValueError(f"unknown task {task!r}")


class FusedAdam(torch.optim.Optimizer):
    """torch.optim.Adam / AdamW semantics (reference train.py:24-31) as ONE kernel over the model's flat
    fp32 parameter buffer, which also rewrites the bf16 shadow the GEMMs read.  `param_groups[0]['lr']`
    is honoured every step, so torch LR schedulers work unchanged.
    max_grad_norm / clip_grad_value: gradient clipping by global norm or by value (one of them; trainer/clip.py).  They are kept
    in `param_groups[0]` (only when set), so state_dict / load_state_dict and checkpoint.save_training_state carry them; the
    launches belong to the step executor (CaptionTrainer), which reads them there before every step."""

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=None, clip_grad_value=None):
        self.model = model
        flat = torch.nn.Parameter(model.flat_params, requires_grad=True)
        flat.grad = model.flat_grads
        super().__init__([flat], dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        set_clip_settings(self, max_grad_norm, clip_grad_value)
        ps = model._ps
        self.exp_avg = torch.zeros_like(ps.flat)
        self.exp_avg_sq = torch.zeros_like(ps.flat)
        self.step_dev = torch.zeros(1, dtype=torch.int32, device=ps.flat.device)
        emb = "cap_decoder.tgt_to_emb.weight"
        a = ps.offsets[emb]
        self.skip = (a, a + (ps.params[emb].numel() + ps.ALIGN - 1) // ps.ALIGN * ps.ALIGN)
        # the reference builds its optimizer over filter(requires_grad) AFTER mode(task) (train.py:24): parameters outside the task's
        # range (caption: matching.*, frozen and never given a gradient; match: the decoder) are neither stepped nor decayed
        self.task = model.f_type
        self.begin, self.end = owned_range(model, self.task)
        # lr / betas / eps / weight decay live in DEVICE memory (read by the kernel): a captured hipGraph or a recorded
        # launch list follows LR schedulers and load_state_dict instead of freezing the values of the recording step
        self.hyper = torch.zeros(8, dtype=torch.float32, device=ps.flat.device)
        self._hyper_host = None
        self.sync_hyper()
        self.pre_state_dict = None      # set by ShardedExchange: all-gather the moments before they are read (collective)
        self._gathered_at = None        # the step count gather_state() last ran at
        # weight matrices stepped INSIDE their weight-gradient GEMMs (enable_dw_fusion): flat ranges registered by desc_for() while the
        # backward of the current step is being enqueued; step_range() then covers only what is left
        self.dw_fusion = False
        self._dw_ranges = []
        self.range_elems = {}
        self._dw_desc = {}
        self._range_tables = {}
        # per-row live table of the token embedding (live_refresh): rows no batch has used are skipped by the multi-range pass
        self._emb = emb
        self._live = None
        self._live_stale = True
        if self.live_rows and ps.flat.is_cuda and ps.g[emb].dim() == 2:
            # made with the optimizer, so that every embedding backward enqueued or recorded from now on marks its rows, whichever
            # executor or task issues it
            self._live = ops.embed_live_table(ps.g[emb], create=True)

    def _hyper_now(self):
        g = self.param_groups[0]
        return (float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"]))

    def sync_hyper(self):
        """Upload the hyper-parameters if a scheduler / user changed them (host check, rare H2D copy).  Called by
        CaptionTrainer.step before every step, outside any capture."""
        h = self._hyper_now()
        if h != self._hyper_host:
            self.hyper[:5].copy_(torch.tensor(h, dtype=torch.float32))
            self._hyper_host = h

    # ---- the optimizer inside the weight-gradient GEMMs (single GPU) ---------------------------------------------------------------
    # A/B switch.  The reference steps every parameter after backward (train.py:125-126); on one GPU nothing sits between a weight's
    # gradient and its update, so the update of every 2-D weight runs in the epilogue of the GEMM that produces the gradient
    # (include/vct_hip.h, vct_gemm_adam): the gradient never goes to HBM and the optimizer's 28 B per parameter move inside MFMA-bound
    # kernels instead of forming a 0.3 ms HBM-bound tail of the step.  What is left (biases, LayerNorm parameters, the embedding
    # table) takes ONE multi-range launch per step_range() call.
    fuse_dw_default = os.environ.get("VCT_FUSE_ADAM", "1") != "0"
    keep_grads = os.environ.get("VCT_FUSE_ADAM_KEEP_GRAD", "0") == "1"      # also store the weight gradients (hooks / inspection)

    def enable_dw_fusion(self, on: bool = True):
        """Called by CaptionTrainer when it owns the whole step (no gradient exchange).  bf16 compute mode on a GPU only."""
        ps = self.model._ps
        ok = bool(on) and ps.compute_dtype == torch.bfloat16 and ps.flat.is_cuda
        self.dw_fusion = ok
        ps.dw_adam = self if ok else None
        self._dw_ranges = []
        return ok

    def set_keep_grads(self, on: bool):
        """Store the weight gradients from the optimizer epilogues as well (CaptionTrainer(keep_weight_grads=...))."""
        if bool(on) != bool(self.keep_grads):
            self.keep_grads = bool(on)
            self._dw_desc.clear()            # the cached epilogue descriptors carry the flag

    # ---- never-used token-embedding rows are not stepped ---------------------------------------------------------------------------
    # A/B switch (VCT_ADAM_LIVE=0: the dense pass).  The embedding table is 30522 x 512 fp32 = 469 MB of the multi-range launch's
    # 470 MB at 30 B per parameter, and a caption batch gives a gradient to the rows of its own tokens only.  A row that never had one
    # has g = m = v = 0, which Adam without weight decay leaves as it is bit for bit (include/vct_hip.h, vct_adam_rows): the pass
    # looks at one flag per row and moves the rows of "every id any batch has used so far" (14 % of the table for bench.py's batch).
    live_rows = os.environ.get("VCT_ADAM_LIVE", "1") != "0"

    def live_refresh(self):
        """Make the embedding's live table exist and be true.  CaptionTrainer.step calls it before every fused step, OUTSIDE any
        recording (the table is device memory the recorded launches read and mark, so recordings replay correctly; the rebuild is a
        188 MB read and must not be part of one).  Host-only check unless the table is new or something else wrote the moments since
        the last row-aware pass: load_state_dict, or a dense pass over the table (another executor or task, the switch).
        model.load_state_dict / checkpoint.load_weights write parameters only -- no moment changes, nothing to rebuild."""
        if not self.live_rows or self.keep_grads:         # (keep_grads: the pass stays dense, the table is brought up to date when it is used again)
            return
        ps = self.model._ps
        g = ps.g[self._emb]
        if g.dim() != 2 or not ps.flat.is_cuda:
            return
        if self._live is None:
            self._live = ops.embed_live_table(g, create=True)        # from here on every embed_bwd into g marks its rows
            self._live_stale = True
        if self._live_stale:
            a, (V, d) = self.skip[0], g.shape
            ops.embed_live_rebuild(self._live, self.exp_avg[a:a + V * d].view(V, d), self.exp_avg_sq[a:a + V * d].view(V, d), g)
            self._live_stale = False

    def _live_rows_for(self, left):
        """{index in left: (origin, row_len, rows, live)} for the pieces of the embedding table, or None (dense).  The table is
        passed on the fused single-GPU path only (this function is reached from the dw_fusion branch of step_range: bf16, no gradient
        exchange, FusedAdam -- the exchange paths, a torch optimizer and fp32 mode never get here) and not with keep_grads; it must be
        current (live_refresh).  Whether a zero row really is a no-op under the hyper-parameters of the step is the kernel's
        decision, taken on the device block."""
        if not self.live_rows or self.keep_grads or self._live is None or self._live_stale:
            return None
        s0, s1 = self.skip
        V, d = self.model._ps.g[self._emb].shape
        rows = {i: (s0, d, V, self._live) for i, (lo, hi, sh) in enumerate(left) if not sh and lo >= s0 and hi <= s1}
        return rows or None

    def begin_step(self):
        """Forget the matrices registered by the previous enqueue of a step (the set is rebuilt as the backward is enqueued)."""
        self._dw_ranges = []

    def desc_for(self, dw: torch.Tensor):
        """ops.L.GemmAdam for the weight whose gradient view `dw` (fp32 [rows, K], rows of one parameter) a GEMM is about to
        produce, and note that this step's step_range() calls must leave its flat range alone.  None: not steppable there."""
        ps = self.model._ps
        off = (dw.data_ptr() - ps.gflat.data_ptr()) // 4
        if not self.dw_fusion or dw.dim() != 2 or dw.dtype != torch.float32 or not (self.begin <= off < self.end):
            return None
        name, base = ps.name_at(off)
        shape = ps.params[name].shape
        rows, K = dw.shape
        if len(shape) != 2 or K != shape[1] or dw.stride(0) != K or dw.stride(1) != 1 or (off - base) % K or name in ps.no_shadow:
            return None
        # the epilogue's own preconditions (vct_gemm's check_desc): 16-byte vectors of gradient / parameter / moments, 8-byte vectors of
        # the shadow.  A matrix that fails them keeps its separate optimizer pass (its range is NOT registered) instead of aborting.
        if K % 4 or off % 4 or (ps.flat.data_ptr() | self.exp_avg.data_ptr() | self.exp_avg_sq.data_ptr() | ps.gflat.data_ptr()) & 15 \
                or ps.cflat.data_ptr() & 7:
            return None
        key = (off, rows, tuple(sorted(ps.packed)))
        ad = self._dw_desc.get(key)
        if ad is None:
            ad = ops.L.GemmAdam()
            ad.param, ad.exp_avg, ad.exp_avg_sq = (t.data_ptr() + 4 * off for t in (ps.flat, self.exp_avg, self.exp_avg_sq))
            ad.shadow, ad.ld_shadow = ps.cflat.data_ptr() + 2 * off, K
            seg = ps.pack_seg(name)
            if seg is not None:
                ad.pk_K, ad.pk_mode, ad.pk_stream, ad.pk_row0 = seg.K, seg.mode, seg.stream, (off - base) // K
                for i in range(4):
                    ad.pk_chunk0[i] = seg.chunk0[i]
            ad.hyper, ad.step = self.hyper.data_ptr(), self.step_dev.data_ptr()
            ad.store_grad = int(self.keep_grads)
            self._dw_desc[key] = ad
        self._dw_ranges.append((off, off + rows * K))
        return ad

    def _left_ranges(self, a: int, b: int):
        """[(begin, end, has_shadow)] of [a, b) minus the matrices registered for this step, split at the shadow-less tensors."""
        cuts = sorted(set((max(x, a), min(y, b)) for x, y in self._dw_ranges if y > a and x < b))
        out, cur = [], a
        for x, y in cuts:
            if x > cur:
                out.append((cur, x))
            cur = max(cur, y)
        if cur < b:
            out.append((cur, b))
        res = []
        s0, s1 = self.skip
        for x, y in out:                      # the embedding table has no bf16 shadow
            for lo, hi, sh in ((x, min(y, s0), True), (max(x, s0), min(y, s1), False), (max(x, s1), y, True)):
                if hi > lo:
                    res.append((lo, hi, sh))
        return res

    @torch.no_grad()
    def step(self, closure=None):
        if not torch.cuda.is_current_stream_capturing():
            self.sync_hyper()
        self.step_range(self.begin, self.end)
        self.finish_ranges()

    # A/B switch: the optimizer's pass writes the stream-order packed weight copies itself (instead of vct_ss_pack launches behind it)
    pack_in_adam = os.environ.get("VCT_ADAM_PACK", "1") != "0"
    # A/B switch: off = the eager transposed shadows by a transpose launch behind the flat pass instead of their weights' own 2-D pass
    adam_2d = os.environ.get("VCT_ADAM2D", "1") != "0"

    @torch.no_grad()
    def step_range(self, a: int, b: int):
        """Adam on flat elements [a, b) only, without advancing the step counter (range-by-range stepping as
        gradient buckets complete); call finish_ranges() after the last range of the step."""
        a, b = max(a, self.begin), min(b, self.end)
        if b <= a:
            return
        lr, b1, b2, eps, wd = self._hyper_now()
        ps = self.model._ps
        bf = ps.compute_dtype != torch.float32
        if self.dw_fusion and self._dw_ranges:
            # the matrices of [a, b) were stepped by their weight-gradient GEMMs (which also wrote their shadows and packed copies): one
            # launch over what is left -- vectors, the embedding table, any matrix whose GEMM did not take the epilogue
            left = self._left_ranges(a, b)
            self.range_elems[(a, b)] = sum(r[1] - r[0] for r in left)        # what this call's launch touches (bench.py: bytes of the bracket)
            table, nseg, pk_parts = ps.adam_pack_table(a, b) if (self.pack_in_adam and ps.packed) else (None, 0, [])
            if left:
                rows = self._live_rows_for(left)
                if rows is None and any(lo < self.skip[1] and hi > self.skip[0] for lo, hi, _sh in left):
                    self._live_stale = True          # a dense pass over the table: the next live_refresh rebuilds
                key = (tuple(left), rows is not None)
                tab = self._range_tables.get(key)
                if tab is None:
                    tab = self._range_tables[key] = ops.adam_ranges_table(left, ps.flat.device, rows)
                ops.adam_step_ranges(ps.flat, ps.gflat, self.exp_avg, self.exp_avg_sq, ps.cflat, tab, lr, b1, b2, eps, wd, self.step_dev,
                                     hyper=self.hyper, pack=(table, nseg) if nseg else None)
            ps.refresh_transposed(a, b, packed_done=pk_parts)
            return
        if a < self.skip[1] and b > self.skip[0]:
            self._live_stale = True                  # a dense pass over the embedding table: the next live_refresh rebuilds
        # 2-D weights with an eager transposed shadow inside the range (W_g^T): their own pass writes the transposed copy too
        fused = []
        if bf and self.adam_2d:
            fused = sorted((x, y, name, t) for name, t, x, y in ps.eager_transposed_in(a, b)      # in flat order
                           if ps.params[name].shape[1] % 64 == 0 and not (x < self.skip[1] and y > self.skip[0]))

        # stream-order packed weight copies (the sample-stationary stack kernels' operand) inside the range: written by the same pass
        table, nseg, pk_parts = ps.adam_pack_table(a, b) if (bf and self.pack_in_adam and ps.packed) else (None, 0, [])

        def flat_range(lo, hi):
            if hi <= lo:
                return
            shadow = ps.cflat[lo:hi] if bf else None
            s0, s1 = max(self.skip[0], lo) - lo, min(self.skip[1], hi) - lo
            ops.adam_step(ps.flat[lo:hi], ps.gflat[lo:hi], self.exp_avg[lo:hi], self.exp_avg_sq[lo:hi], shadow, lr, b1, b2, eps, wd,
                          self.step_dev, (s0, s1) if s1 > s0 else (0, 0), bump=False, hyper=self.hyper,
                          pack=(table, nseg, lo) if nseg else None)
        cur = a
        for x, y, name, t in fused:
            flat_range(cur, x)
            shape = ps.params[name].shape
            ops.adam_step_2d(ps.flat[x:y].view(shape), ps.gflat[x:y].view(shape), self.exp_avg[x:y].view(shape),
                             self.exp_avg_sq[x:y].view(shape), ps.cflat[x:y].view(shape), t, lr, b1, b2, eps, wd, self.step_dev,
                             hyper=self.hyper)
            cur = y
        flat_range(cur, b)
        if bf:
            ps.refresh_transposed(a, b, skip=[name for _x, _y, name, _t in fused], packed_done=pk_parts)   # other eager copies follow the shadow this pass rewrote

    @torch.no_grad()
    def finish_ranges(self):
        ops.adam_bump(self.step_dev)
        self.model._ps.optimizer_stepped()

    def zero_grad(self, set_to_none: bool = True):
        pass   # the backward schedule OVERWRITES every gradient (no accumulation across backward calls on the fast path)

    # ---- checkpointing (checkpoint.save_training_state): moments and step live outside torch's per-param state ----
    def gather_state(self):
        """Data-parallel runs with a sharded optimizer: bring every rank's Adam moments up to date on this rank (a COLLECTIVE --
        every rank calls it; checkpoint.save_training_state does).  No-op otherwise."""
        if self.pre_state_dict is not None:
            self.pre_state_dict()
        self._gathered_at = int(self.step_dev.item())

    def state_dict(self):
        if self.pre_state_dict is not None and self._gathered_at != int(self.step_dev.item()):
            # the moments of the shards other ranks own are stale here: gathering them is a collective and must not hide in a call
            # that a single rank may make (`if rank == 0: save(...)` would hang in it)
            raise RuntimeError("FusedAdam.state_dict() under a sharded exchange: call optimizer.gather_state() on EVERY rank first "
                               "(checkpoint.save_training_state does), then state_dict() on the rank(s) that write")
        sd = super().state_dict()
        ps = self.model._ps
        sd["vct_fused_adam"] = {"exp_avg": self.exp_avg.detach().clone(), "exp_avg_sq": self.exp_avg_sq.detach().clone(),
                                "step": int(self.step_dev.item()), "numel": ps.flat.numel(),
                                "layout": [(k, int(ps.offsets[k])) for k in ps.params]}
        return sd

    def load_state_dict(self, state_dict):
        sd = dict(state_dict)
        fused = sd.pop("vct_fused_adam", None)
        if fused is None:
            raise ValueError("not a FusedAdam state (no 'vct_fused_adam' entry)")
        ps = self.model._ps
        if fused["numel"] != ps.flat.numel() or [tuple(x) for x in fused["layout"]] != [(k, int(ps.offsets[k])) for k in ps.params]:
            raise ValueError("optimizer state was saved for a different parameter layout")
        super().load_state_dict(sd)
        self.exp_avg.copy_(fused["exp_avg"])
        self.exp_avg_sq.copy_(fused["exp_avg_sq"])
        self.step_dev.fill_(fused["step"])
        self._live_stale = True       # the moments were written from outside: the live table is rebuilt before the next fused step
        self._gathered_at = None      # (a restored step count says nothing about the other ranks' shards: gather_state() again before a save)
        self.sync_hyper()


def set_clip_settings(optimizer, max_grad_norm=None, clip_grad_value=None):
    """Validate the clipping settings and write those that are set into optimizer.param_groups[0] (any optimizer kind)."""
    check_clip_settings(max_grad_norm, clip_grad_value)
    for key, v in zip(CLIP_KEYS, (max_grad_norm, clip_grad_value)):
        if v is not None:
            optimizer.param_groups[0][key] = float(v)


def build_optimizer(train_cfg: dict, model):
    """Optimizer + scheduler factory with the reference's config surface (train.py:20-49).  The
    optimizer sees ONE parameter -- the flat fp32 buffer, whose .grad is the flat gradient buffer --
    so Adam is a single fused multi-tensor kernel instead of ~70 small ones.
    Beyond the reference: the optional train.optimizer.max_grad_norm / clip_grad_value (gradient clipping, trainer/clip.py)."""
    oc = train_cfg["optimizer"]

    def flat():      # what a torch optimizer steps (FusedAdam makes its own)
        p = torch.nn.Parameter(model.flat_params, requires_grad=True)
        p.grad = model.flat_grads
        return [p]
    if oc["name"] == "adam":
        if model.flat_params.is_cuda:
            opt = FusedAdam(model, lr=oc["learning_rate"], betas=tuple(oc["beta"]), weight_decay=oc.get("weight_decay", 0) or 0.0)
        elif oc.get("weight_decay", 0) == 0:
            opt = torch.optim.Adam(flat(), lr=oc["learning_rate"], betas=tuple(oc["beta"]))
        else:
            opt = torch.optim.AdamW(flat(), lr=oc["learning_rate"], betas=tuple(oc["beta"]), weight_decay=oc["weight_decay"])
    elif oc["name"] == "sgd":
        opt = torch.optim.SGD(flat(), lr=oc["learning_rate"], momentum=oc["momentum"])
    else:
        raise ValueError("Do not support optimizer: {}".format(oc["name"]))
    set_clip_settings(opt, oc.get("max_grad_norm"), oc.get("clip_grad_value"))
    sched = None
    sc = oc.get("lr_scheduler")
    if sc:
        if sc["name"] == "CosineAnnealingLR":
            sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=sc["T_max"], eta_min=sc["eta_min"])
        elif sc["name"] == "ReduceLROnPlateau":
            sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, patience=sc["patience"])
        else:
            raise ValueError("Do not support lr_scheduler: {}".format(sc["name"]))
    return opt, sched
