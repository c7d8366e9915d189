"""What the encoder and decoder engines share: side-stream plumbing, weight-gradient grouping, the attention / LayerNorm /
feed-forward blocks and the sample-stationary stack."""
from typing import Dict

import os

import torch

from .. import ops
from .params import ParamSet, _Buf

ENC_SITE, DEC_SITE, EMB_SITE = 0, 1000, 999
ENC_IN_SITE = 998  # the Dropout behind the encoder's input LayerNorm (do_norm): below EMB_SITE, above every encoder layer's ENC_SITE + 16 l + 1..4
SAMPLE_SITE = 997  # the counter hash behind sampled decoding's uniforms (csrc/vct_sample.hip, SMP_SITE): below ENC_IN_SITE, above every encoder layer's sites
DMEM_SYNC = 0      # named sync point (ops.sync_record / sync_wait): d(memory) is final on the main stream


_CUS = {}


def _cu_count(dev) -> int:
    n = _CUS.get(dev)
    if n is None:
        n = _CUS[dev] = torch.cuda.get_device_properties(dev).multi_processor_count if dev.type == "cuda" else 0
    return n


class _StackBase:
    def __init__(self, ps: ParamSet, prefix: str, cfg: dict, seed: torch.Tensor):
        self.ps, self.pre, self.cfg, self.seed = ps, prefix, cfg, seed
        self.dev, self.dt = ps.device, ps.compute_dtype
        self.bufs: Dict[tuple, _Buf] = {}
        self.p_drop = 0.0
        self._ws = None
        self._ln_pending = []
        self._dw_pending = []
        self._kv_prefetched = None
        self._kv_inplace = set()
        self._prefix = None

    # parameter access: compute-dtype weight, fp32 vector, fp32 gradient
    def W(self, k): return self.ps.c[self.pre + k]
    def WT(self, k): return self.ps.want_transposed(self.pre + k)      # [in, out] copy, kept in step with the shadow
    def F(self, k): return self.ps.params[self.pre + k].data
    def G(self, k): return self.ps.g[self.pre + k]

    def drop(self, site):
        return (self.seed, site, self.p_drop) if self.p_drop > 0.0 else None

    def gemm_ws(self):
        """Split-K scratch of the main stream (partials + zeroed tile counters)."""
        if self._ws is None:
            self._ws = ops.GemmScratch(self.dev)
        return self._ws

    # ---- weight-gradient GEMMs: grouped per layer, on a side HIP stream ---------------------------
    # dW = dY^T X only depends on dY (produced by the dX chain) and X (saved), and nothing downstream in backward
    # reads it.  A layer's 4-7 weight gradients are small (16-128 output tiles each): they are queued while the
    # layer's dX chain runs and issued as ONE grouped launch (ops.gemm_grouped) on a second stream, where they
    # overlap the next layer's dX chain.  The two big ones (generator) go out immediately, alone.
    overlap_dw = True
    group_dw = True
    overlap_kv = True      # cross-attention K/V projections and d(memory) accumulation off the critical path
    defer_gen_dw = True    # single GPU: vocabulary weight gradient at the end of the main stream's tail (A/B switch)

    @property
    def side(self):
        """The model's side stream (None until something needed it)."""
        return self.ps.ctx.side

    def ensure_side(self):
        ctx = self.ps.ctx
        if ctx.side is None:
            # Normal priority.  (Round 5 measured a HIGH-priority side stream: without a gradient exchange the encoder backward's short
            # kernels win freed slots beside the vocabulary weight gradient -- step -0.8 % in three same-box pairs, 0 in a fourth, i.e.
            # inside the run-to-run spread -- but WITH an exchange, collectives in flight on the communicator's stream, every kernel of
            # the step is stretched: world size 1, sharded exchange, 2.88 -> 4.69 ms.  Not worth a stream whose effect depends on what
            # else is in flight: dropped.)
            ctx.side = torch.cuda.Stream(device=self.dev)
            ctx.side_ws = ops.GemmScratch(self.dev)
        return ctx.side

    def _on_side(self, fn):
        if not (self.overlap_dw and self.dev.type == "cuda"):
            return fn(self.gemm_ws())
        ctx = self.ps.ctx
        self.ensure_side()
        cur = torch.cuda.current_stream()
        if cur == ctx.side:               # already running on the side stream (encoder backward beside the decoder's tail)
            return fn(ctx.side_ws)
        ops.stream_wait(ctx.side, cur)
        with torch.cuda.stream(ctx.side):
            return fn(ctx.side_ws)

    def dw_gemm(self, dy, x, dw, *, bias_grad=None, m_valid=None, tag=None):
        """dw[M,N] (fp32 gradient view) = dy^T x, bias_grad[M] = column sums of dy."""
        ad = self.dw_adam_desc(dy, dw)
        if self.group_dw and m_valid is None and tag is None and dy.dtype == torch.bfloat16:
            self._dw_pending.append((dy, x, dw, bias_grad, ad))
            if len(self._dw_pending) == ops.L.GEMM_GROUP_MAX:
                self.flush_dw()
            return
        self._on_side(lambda ws: ops.gemm(dy, x, dw, ta=True, tb=False, bias_grad=bias_grad, m_valid=m_valid, tag=tag,
                                          workspace=ws, adam=ad))

    def dw_adam_desc(self, dy, dw):
        """Epilogue descriptor (ops.L.GemmAdam) when the optimizer steps this weight inside the GEMM that produces its gradient
        `dw` (single GPU, trainer.FusedAdam.enable_dw_fusion), else None."""
        opt = self.ps.dw_adam
        if opt is None or dy.dtype != torch.bfloat16 or self.dev.type != "cuda":
            return None
        return opt.desc_for(dw)

    def flush_dw(self, main: bool = False):
        """Issue the queued weight-gradient GEMMs as one grouped launch (side stream, or the current one if `main`)."""
        if self._dw_pending:
            items, self._dw_pending = self._dw_pending, []
            if main:
                ops.gemm_grouped(items, self.gemm_ws())
            else:
                self._on_side(lambda ws: ops.gemm_grouped(items, ws))

    def flush_dw_across(self, other):
        """Issue the queued weight-gradient group on the stream `other` (behind everything enqueued so far on the current one) instead
        of in line on the current stream: the encoder backward runs as ONE serial chain on the side stream, and a layer's group in
        the middle of that chain (72 us alone, 187 us beside the vocabulary dW) delays every kernel behind it, while the main
        stream idles at the end of the step (profiles/r05_step_timeline_list.txt).  The group only needs this layer's dY / X."""
        if not self._dw_pending:
            return
        cur = torch.cuda.current_stream()
        if other is None or other == cur or not (self.overlap_dw and self.dev.type == "cuda"):
            return self.flush_dw()
        items, self._dw_pending = self._dw_pending, []
        ops.stream_wait(other, cur)
        with torch.cuda.stream(other):
            ops.gemm_grouped(items, self.gemm_ws() if other != self.ps.ctx.side else self.ps.ctx.side_ws)

    def bucket_on_side(self, bucket_ready, *args):
        """Hand a finished gradient bucket to `bucket_ready` WITHOUT stalling the dX chain: the hook runs with the
        side stream current, after that stream has been ordered behind everything enqueued so far on the main
        stream -- an all-reduce issued from the hook waits for this bucket's weight gradients (side stream) and
        LayerNorm/bias gradients (main stream) while the main stream goes straight on to the next layer."""
        self.flush_dw()
        side = self.ps.ctx.side
        if side is None or not self.overlap_dw or torch.cuda.current_stream() == side:
            return bucket_ready(*args)
        ops.stream_wait(side, None)
        with torch.cuda.stream(side):
            return bucket_ready(*args)

    def join_side(self):
        """Main stream waits for every weight-gradient GEMM issued so far (before a gradient bucket is
        handed to the exchange / the optimizer)."""
        self.flush_dw()
        side = self.ps.ctx.side
        if side is not None and self.overlap_dw and torch.cuda.current_stream() != side:
            ops.stream_wait(None, side)

    def buf(self, key) -> _Buf:
        """The engine's buffer set (`key` = the shape configuration, kept for diagnostics only: every configuration
        shares one set of grow-only allocations, see _Buf)."""
        b = self.bufs.get("all")
        if b is None:
            b = self.bufs["all"] = _Buf(self.dev, self.ps.ctx)
        return b

    # ---- shared sub-blocks -------------------------------------------------------------------
    def _attn_block_fwd(self, b, tag, lp, x, kv_src, Bn, Lq, Lk, causal, key_pad, site, self_attn=True):
        """x:[Mq,d] queries source; kv_src:[Mk,d].  Returns (a = out_proj(attn) [Mq,d])."""
        d, H = self.cfg["d"], self.cfg["nhead"]
        Mq, Mk = x.shape[0], kv_src.shape[0]
        if self_attn:
            qkv = b.get(tag + "qkv", (Mq, 3 * d), self.dt)
            ops.gemm(x, self.W(lp + "in_proj_weight"), qkv, bias=self.F(lp + "in_proj_bias"))
            q, k, v = qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:]
        else:
            q = b.get(tag + "q", (Mq, d), self.dt)
            ops.gemm(x, self.W(lp + "in_proj_weight")[:d], q, bias=self.F(lp + "in_proj_bias")[:d])
            kv = self._cross_kv(b, tag, lp, kv_src)
            k, v = kv[:, :d], kv[:, d:]
        o = b.get(tag + "o", (Mq, d), self.dt)
        ops.attn_fwd(q, k, v, o, Bn, H, Lq, Lk, causal=causal, key_pad=key_pad, dropout=self.drop(site))
        a = b.get(tag + "a", (Mq, d), self.dt)
        ops.gemm(o, self.W(lp + "out_proj.weight"), a, bias=self.F(lp + "out_proj.bias"))
        return a

    def _attn_ln_fwd(self, b, tag, ntag, lp, np_, x, kv_src, Bn, Lq, Lk, causal, key_pad, site, site_ln, self_attn=True):
        """y = LayerNorm(x + dropout(out_proj(MHA(x, kv_src)))) of one attention block; saves o, a, mean, rstd for the backward.
        (Two fused forms of this block -- attention core + out_proj + add-LayerNorm as one launch, and out_proj + add-LayerNorm as one
        row-complete launch -- were built in rounds 3/4, measured slower in the step and removed in round 5: git tag
        archive/r5-off-kernels)"""
        a = self._attn_block_fwd(b, tag, lp, x, kv_src, Bn, Lq, Lk, causal, key_pad, site, self_attn=self_attn)
        return self._ln_fwd(b, ntag, np_, a, x, site_ln)

    def _cross_kv(self, b, tag, lp, mem):
        """K/V projection of the encoder memory for one cross-attention block.  It depends on the memory only, so
        prefetch_cross_kv() issues it for every layer on the side stream at the start of the decoder stack, off the
        critical path; here it is either picked up (after joining that stream) or computed in place."""
        d = self.cfg["d"]
        kv = b.get(tag + "kv", (mem.shape[0], 2 * d), self.dt)
        if self._kv_prefetched and tag not in self._kv_inplace:
            if self._kv_prefetched == "pending":
                self.join_side()
                self._kv_prefetched = "joined"
        else:
            ops.gemm(mem, self.W(lp + "in_proj_weight")[d:], kv, bias=self.F(lp + "in_proj_bias")[d:])
        return kv

    def prefetch_cross_kv(self, b, mem, tags_lps):
        if not self.overlap_kv or not tags_lps:
            return
        d = self.cfg["d"]
        for tag, lp in tags_lps:
            kv = b.get(tag + "kv", (mem.shape[0], 2 * d), self.dt)
            self._on_side(lambda ws, kv=kv, lp=lp: ops.gemm(mem, self.W(lp + "in_proj_weight")[d:], kv, bias=self.F(lp + "in_proj_bias")[d:]))
        self._kv_prefetched = "pending"

    def _attn_block_bwd(self, b, tag, lp, da, x, kv_src, Bn, Lq, Lk, causal, key_pad, site, self_attn, ds_res,
                        dkv_out=None, dkv_accumulate=False):
        """da: grad of out_proj output (dropout-masked).  Returns dx = grad wrt x (+ ds_res)."""
        d, H = self.cfg["d"], self.cfg["nhead"]
        Mq, Mk = x.shape[0], kv_src.shape[0]
        o = b.t[tag + "o"]
        d_o = b.get(tag + "d_o", (Mq, d), self.dt)
        ops.gemm(da, self.W(lp + "out_proj.weight"), d_o, ta=False, tb=False)
        self.dw_gemm(da, o, self.G(lp + "out_proj.weight"), bias_grad=self.G(lp + "out_proj.bias"))
        dx = b.get(tag + "dx", (Mq, d), self.dt)
        if self_attn:
            qkv = b.t[tag + "qkv"]
            dqkv = b.get(tag + "dqkv", (Mq, 3 * d), self.dt)
            ops.attn_bwd(qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], d_o, dqkv[:, :d], dqkv[:, d:2 * d], dqkv[:, 2 * d:],
                         Bn, H, Lq, Lk, causal=causal, key_pad=key_pad, dropout=self.drop(site))
            ops.gemm(dqkv, self.W(lp + "in_proj_weight"), dx, ta=False, tb=False, addend=ds_res)
            self.dw_gemm(dqkv, x, self.G(lp + "in_proj_weight"), bias_grad=self.G(lp + "in_proj_bias"))
        else:
            q, kv = b.t[tag + "q"], b.t[tag + "kv"]
            dq = b.get(tag + "dq", (Mq, d), self.dt)
            dkv = b.get(tag + "dkv", (Mk, 2 * d), self.dt)
            ops.attn_bwd(q, kv[:, :d], kv[:, d:], d_o, dq, dkv[:, :d], dkv[:, d:], Bn, H, Lq, Lk, causal=causal,
                         key_pad=key_pad, dropout=self.drop(site))
            ops.gemm(dq, self.W(lp + "in_proj_weight")[:d], dx, ta=False, tb=False, addend=ds_res)
            self.dw_gemm(dq, x, self.G(lp + "in_proj_weight")[:d], bias_grad=self.G(lp + "in_proj_bias")[:d])
            # d(memory) is only read by the encoder backward: accumulate it on the side stream (in layer order)
            run = self._on_side if self.overlap_kv else (lambda fn: fn(None))
            run(lambda ws: ops.gemm(dkv, self.W(lp + "in_proj_weight")[d:], dkv_out, ta=False, tb=False,
                                    addend=dkv_out if dkv_accumulate else None))
            self.dw_gemm(dkv, kv_src, self.G(lp + "in_proj_weight")[d:],
                         bias_grad=self.G(lp + "in_proj_bias")[d:])
        return dx

    def _ln_fwd(self, b, tag, np_, x, res, site):
        M, d = x.shape
        y = b.get(tag + "y", (M, d), self.dt)
        ops.add_ln_fwd(x, res, self.F(np_ + "weight"), self.F(np_ + "bias"), y, b.get(tag + "mean", (M,), torch.float32),
                       b.get(tag + "rstd", (M,), torch.float32), dropout=self.drop(site) if site is not None else None)
        return y

    def _ln_ln_fwd(self, b, tag, np_, x, res, site, tag2, np2):
        """The last layer's closing norm and the stack-final norm in one launch: returns (y, y2)."""
        M, d = x.shape
        y, y2 = b.get(tag + "y", (M, d), self.dt), b.get(tag2 + "y", (M, d), self.dt)
        ops.add_ln_ln_fwd(x, res, self.F(np_ + "weight"), self.F(np_ + "bias"), y, b.get(tag + "mean", (M,), torch.float32),
                          b.get(tag + "rstd", (M,), torch.float32), self.F(np2 + "weight"), self.F(np2 + "bias"), y2,
                          b.get(tag2 + "mean", (M,), torch.float32), b.get(tag2 + "rstd", (M,), torch.float32),
                          dropout=self.drop(site) if site is not None else None)
        return y, y2

    def _ln_bwd(self, b, tag, np_, dy, x, res, site):
        """Returns (ds, dxo): gradient of the pre-norm sum and its dropout-masked copy.  The column
        reduction of the dgamma/dbeta partials is deferred: flush_ln_grads() does all of them in one launch."""
        M, d = x.shape
        ds = b.get(tag + "ds", (M, d), self.dt)
        drop = self.drop(site) if site is not None else None
        dxo = b.get(tag + "dxo", (M, d), self.dt) if drop is not None else ds
        ws = b.get(tag + "ln_ws", (2 * ops.ln_ws_rows(M) * d,), torch.float32)     # one per LayerNorm (kept until the flush)
        ops.add_ln_bwd(dy, x, res, self.F(np_ + "weight"), b.t[tag + "mean"], b.t[tag + "rstd"], ds, dxo,
                       None, None, ws, dropout=drop)
        self._ln_pending.append((ws.data_ptr(), self.G(np_ + "weight").data_ptr(), self.G(np_ + "bias").data_ptr(),
                                 ops.ln_ws_rows(M)))
        return ds, dxo

    fuse_ln_ln_bwd = os.environ.get("VCT_LN_LN_BWD", "1") != "0"      # A/B switch

    def _ln_ln_bwd(self, b, tag2, np2, dy2, y, tag, np_, x, res, site):
        """The stack-final norm's backward and the top layer's closing norm's backward in ONE launch (ops.add_ln_ln_bwd; bit-identical
        to _ln_bwd(final) followed by _ln_bwd(layer)).  Returns (ds, dxo) of the layer norm."""
        M, d = x.shape
        ds = b.get(tag + "ds", (M, d), self.dt)
        drop = self.drop(site) if site is not None else None
        dxo = b.get(tag + "dxo", (M, d), self.dt) if drop is not None else ds
        rows = ops.ln_ws_rows(M)
        ws2 = b.get(tag2 + "ln_ws", (2 * rows * d,), torch.float32)
        ws = b.get(tag + "ln_ws", (2 * rows * d,), torch.float32)
        ops.add_ln_ln_bwd(dy2, y, self.F(np2 + "weight"), b.t[tag2 + "mean"], b.t[tag2 + "rstd"], ws2, x, res, self.F(np_ + "weight"),
                          b.t[tag + "mean"], b.t[tag + "rstd"], ds, dxo, ws, dropout=drop)
        for w_, n_ in ((ws2, np2), (ws, np_)):
            self._ln_pending.append((w_.data_ptr(), self.G(n_ + "weight").data_ptr(), self.G(n_ + "bias").data_ptr(), rows))
        return ds, dxo

    def flush_ln_grads(self, b):
        """One launch: dgamma/dbeta of every LayerNorm whose backward ran since the last flush."""
        if not self._ln_pending:
            return
        key = tuple(self._ln_pending)
        tab = b.t.get(("ln_table", key))
        if tab is None:       # pointers are static per shape configuration: the table is uploaded once
            tab = torch.tensor(self._ln_pending, dtype=torch.int64).to(self.dev)
            b.t[("ln_table", key)] = tab
        ops.ln_param_finalize_batched(tab, len(self._ln_pending), self.cfg["d"])
        self._ln_pending = []

    # ---- ONE launch per layer: the sample-stationary forward (csrc/vct_layer_ss.hip) ---------------------------------------
    # A/B switch.  bf16, d = 512 / 8 heads, rows per sample <= 32, memory rows <= 16: every layer of the stack is one launch in
    # which a workgroup keeps its sample in LDS and streams the layer's weights (a stream-order packed second shadow) from L2.
    # It saves the tensors and draws the dropout streams of the unfused kernels: the backward schedule is unchanged behind it.
    fuse_layers = os.environ.get("VCT_FUSE_LAYERS", "1") != "0"

    def _ss_ok(self, Lr: int, Lm: int, Bn: int) -> bool:
        """One workgroup per sample streams ALL of a layer's weights: it pays while the samples fit the CUs in one round (cfg-B:
        256 samples on 256 CUs, forward bracket 0.52 vs 0.55 ms unfused); at a per-GPU batch of 1024 the tiled GEMMs amortise the
        weights over 4864+ rows and win (1.39 vs 1.84 ms)."""
        c = self.cfg
        if not (self.fuse_layers and self.dev.type == "cuda" and c["activation"] in ("gelu", "relu")):
            return False
        if Bn > _cu_count(self.dev) * 5 // 4:
            return False
        return ops.layer_ss_supported(self.dt, c["d"], c["nhead"], c["ff"], Lr, Lm)

    def _ss_stream(self, lps, cross: bool, lead=None):
        """The packed weight stream of the stack's layers `lps` (blocks in the kernel's consumption order, layer after layer); lead =
        name of a 512 x 512 weight the kernel's prologue consumes first (the encoder's unify Linear)."""
        ff = self.cfg["ff"]

        def one(lp):
            P = self.pre + lp
            names = [P + "self_attn.in_proj_weight", P + "self_attn.out_proj.weight", P + "linear1.weight", P + "linear2.weight"]
            if cross:
                names += [P + "multihead_attn.in_proj_weight", P + "multihead_attn.out_proj.weight"]

            def blocks():
                c, out, at = self.ps.c, [], 0
                mats = [(c[P + "self_attn.in_proj_weight"], 3), (c[P + "self_attn.out_proj.weight"], 1)]
                if cross:
                    mats += [(c[P + "multihead_attn.in_proj_weight"], 3), (c[P + "multihead_attn.out_proj.weight"], 1)]
                for w, nb in mats:
                    for i in range(nb):
                        out.append((w[512 * i:512 * (i + 1)], 8, at)); at += 8
                # feed-forward, software-pipelined: linear1 block 0 | for j: linear1 block j+1 (its K steps carry chunk j's GELU), linear2 K slice j
                w1, w2 = c[P + "linear1.weight"], c[P + "linear2.weight"]
                nj = ff // 512
                out.append((w1[0:512], 8, at)); at += 8
                for j in range(nj):
                    if j + 1 < nj:
                        out.append((w1[512 * (j + 1):512 * (j + 2)], 8, at)); at += 8
                    out.append((w2[:, 512 * j:512 * (j + 1)], 8, at)); at += 8
                return out
            return names, blocks
        parts = [one(lp) for lp in lps]
        if lead is not None:
            parts.insert(0, ([self.pre + lead], lambda: [(self.ps.c[self.pre + lead][0:512], 8, 0)]))
        return self.ps.want_packed(self.pre + lps[0] + f"x{len(lps)}" + (lead or ""), parts)

    def _ss_stream_bwd(self, lps):
        """The packed TRANSPOSED weight stream of the self-attention + feed-forward layers `lps` (processing order of the backward:
        top layer first) for vct_layer_ss_bwd: [linear2^T block j | linear1^T K slice j] x ff/512 | out_proj^T | in_proj^T."""
        ff = self.cfg["ff"]

        def one(lp):
            P = self.pre + lp
            names = [P + "self_attn.in_proj_weight", P + "self_attn.out_proj.weight", P + "linear1.weight", P + "linear2.weight"]

            def blocks():
                c, out, at = self.ps.c, [], 0
                w1, w2 = c[P + "linear1.weight"], c[P + "linear2.weight"]
                for j in range(ff // 512):
                    out.append((w2[:, 512 * j:], 8, at, True)); at += 8
                    out.append((w1[512 * j:512 * (j + 1)], 8, at, True)); at += 8
                out.append((c[P + "self_attn.out_proj.weight"], 8, at, True)); at += 8
                out.append((c[P + "self_attn.in_proj_weight"], 24, at, True)); at += 24
                return out
            return names, blocks
        return self.ps.want_packed(self.pre + lps[0] + f"bwd{len(lps)}", [one(lp) for lp in lps])

    # The activation-gradient chain of a self-attention + feed-forward stack as ONE launch (csrc/vct_layer_ss_bwd.hip): OFF by default.
    # Measured at cfg-B (round 4, same box): the launch takes 236 us ALONE for the two encoder layers against 253 us for the 14 unfused
    # launches alone -- but it takes whole compute units (152 KB of LDS per workgroup), so nothing runs beside it, while the unfused
    # chain shares the chip with the vocabulary weight gradient and the optimizer's pass in the step's tail: step 2.40-2.42 ms with it
    # (beside the tail, or alone on the main stream ahead of the optimizer) against 2.24-2.26 ms without.  VCT_FUSE_BWD=1 enables it.
    fuse_bwd = os.environ.get("VCT_FUSE_BWD", "0") == "1"

    def _stack_ss_bwd(self, b, lps, tags, sites0, dy, dx, Bn, Lr, *, ln_tag, ln_name, final, kpm=None, causal=False):
        """Gradient of the stack input from the gradient `dy` of the (final-normed) stack output: ONE launch; queues the layers' weight-
        gradient GEMMs (grouped, one launch per layer) and the LayerNorm parameter partials behind it.  lps / tags / sites0 in FORWARD
        order (bottom layer first)."""
        d, ff, H = self.cfg["d"], self.cfg["ff"], self.cfg["nhead"]
        M = Bn * Lr
        f32 = torch.float32
        order = list(reversed(range(len(lps))))
        wpk, firsts = self._ss_stream_bwd([lps[l] for l in order])
        per = ops.layer_ss_bwd_stream_chunks(ff)
        descs, after = [], []
        for k, l in enumerate(order):
            lp, tag, site = lps[l], tags[l], sites0[l]

            def nb(t, name):
                ws = b.get(t + "ss_ws", (Bn * 2 * d,), f32)
                self._ln_pending.append((ws.data_ptr(), self.G(name + "weight").data_ptr(), self.G(name + "bias").data_ptr(), Bn))
                return (self.F(name + "weight"), b.t[t + "mean"], b.t[t + "rstd"], ws)
            nf = nb("nf.", final) if k == 0 else None
            n3 = nb(tag + ln_tag, lp + ln_name)
            n1 = nb(tag + "n1.", lp + "norm1.")
            df, dhpre = b.get(tag + ln_tag + "dxo", (M, d), self.dt), b.get(tag + "ff.dhpre", (M, ff), self.dt)
            da, dqkv = b.get(tag + "n1.dxo", (M, d), self.dt), b.get(tag + "sa.dqkv", (M, 3 * d), self.dt)
            x, x1 = b.t[tag + "x"], b.t[tag + "n1.y"]
            descs.append(ops.layer_ss_bwd_desc(
                B=Bn, Lr=Lr, wpk=wpk[firsts[k] * ops.SS_CHUNK:], nchunks=per, ff=ff, act=self.cfg["activation"], H=H,
                x=x, qkv=b.t[tag + "sa.qkv"], a=b.t[tag + "sa.a"], x1=x1, hpre=b.t[tag + "ff.hpre"], f=b.t[tag + "ff.f"],
                n1=n1, n3=n3, nf=nf, y_last=b.t["x_last"] if k == 0 else None, dy=dy if k == 0 else None,
                dx=dx if k == len(order) - 1 else None, outs=(df, dhpre, da, dqkv),
                sites=(site + 1, site + 2, site + 3, site + 4), causal=causal, key_pad=kpm,
                seed=self.seed if self.p_drop > 0.0 else None, p_drop=self.p_drop))
            sa = lp + "self_attn."
            after.append([(df, b.t[tag + "ff.h"], lp + "linear2."), (dhpre, x1, lp + "linear1."), (da, b.t[tag + "sa.o"], sa + "out_proj."),
                          (dqkv, x, sa + "in_proj_")])
        ops.layer_ss_bwd(descs)
        return order, after

    def _stack_ss(self, b, lps, tags, x, Bn, Lr, sites0, *, ln_tag, ln_name, final, mem=None, Lm=0, causal=False, kpm=None,
                  frontend=None, embed=None):
        """The layers `lps` (buffer tags `tags`, dropout site bases `sites0`) on input x [Bn*Lr, d] in ONE launch per four layers.
        ln_tag / ln_name: buffer tag and parameter name of a layer's closing norm ('n2.' / 'norm2.' encoder, 'n3.' / 'norm3.' decoder);
        final = parameter prefix of the stack-final norm.  Returns (last layer's output, final-norm output)."""
        d, ff, H = self.cfg["d"], self.cfg["ff"], self.cfg["nhead"]
        M, cross = Bn * Lr, mem is not None
        f32 = torch.float32
        wpk, firsts = self._ss_stream(lps, cross, lead="unify.0.weight" if frontend is not None else None)
        if frontend is not None:
            firsts = firsts[1:]                  # (the kernel's prologue reads the unify block from the head of the stream itself)
        per = ops.layer_ss_stream_chunks(ff, cross)
        descs, y, y2 = [], x, None
        for l, (lp, tag, site) in enumerate(zip(lps, tags, sites0)):
            b.t[tag + "x"] = y

            def norm(t, name):
                return (self.F(name + "weight"), self.F(name + "bias"), b.get(t + "y", (M, d), self.dt), b.get(t + "mean", (M,), f32),
                        b.get(t + "rstd", (M,), f32))
            sa, st = lp + "self_attn.", tag + "sa."
            bias = {"qkv": self.F(sa + "in_proj_bias"), "o": self.F(sa + "out_proj.bias"), "l1": self.F(lp + "linear1.bias"),
                    "l2": self.F(lp + "linear2.bias")}
            kw = {}
            if cross:
                ca, ct = lp + "multihead_attn.", tag + "ca."
                bias.update(cq=self.F(ca + "in_proj_bias")[:d], ckv=self.F(ca + "in_proj_bias")[d:], co=self.F(ca + "out_proj.bias"))
                kw = dict(cross=(b.get(ct + "q", (M, d), self.dt), b.get(ct + "kv", (Bn * Lm, 2 * d), self.dt), b.get(ct + "o", (M, d), self.dt),
                                 b.get(ct + "a", (M, d), self.dt)),
                          n2=norm(tag + "n2.", lp + "norm2."), mem=mem, Lm=Lm)
                sites = (site + 1, site + 2, site + 3, site + 4, site + 5, site + 6)
            else:
                sites = (site + 1, site + 2, 0, 0, site + 3, site + 4)
            nl = norm(tag + ln_tag, lp + ln_name)
            nf = norm("nf.", final) if l == len(lps) - 1 else None
            descs.append(ops.layer_ss_desc(
                B=Bn, Lr=Lr, x=y, wpk=wpk[(firsts[l] if l else 0) * ops.SS_CHUNK:], nchunks=per, ff=ff, act=self.cfg["activation"], H=H, bias=bias,
                sa=(b.get(st + "qkv", (M, 3 * d), self.dt), b.get(st + "o", (M, d), self.dt), b.get(st + "a", (M, d), self.dt)),
                n1=norm(tag + "n1.", lp + "norm1."),
                ffn=(b.get(tag + "ff.hpre", (M, ff), self.dt), b.get(tag + "ff.h", (M, ff), self.dt), b.get(tag + "ff.f", (M, d), self.dt)),
                n3=nl, nf=nf, causal=causal, key_pad=kpm, seed=self.seed, p_drop=self.p_drop, sites=sites,
                frontend=frontend if l == 0 else None, embed=embed if l == 0 else None, **kw))
            y, y2 = nl[2], (nf[2] if nf is not None else None)
        tag_ = "ss_dec" if cross else "ss_enc"
        ops.tap(tag_, 0)
        ops.layer_ss_fwd(descs)
        ops.tap(tag_, 1)
        return y, y2

    def _ffn_fwd(self, b, tag, lp, x, site):
        M, d = x.shape
        ff = self.cfg["ff"]
        hpre = b.get(tag + "hpre", (M, ff), self.dt)
        h = b.get(tag + "h", (M, ff), self.dt)
        ops.gemm(x, self.W(lp + "linear1.weight"), h, bias=self.F(lp + "linear1.bias"), act=self.cfg["activation"],
                 preact=hpre, dropout=self.drop(site))
        f = b.get(tag + "f", (M, d), self.dt)
        ops.gemm(h, self.W(lp + "linear2.weight"), f, bias=self.F(lp + "linear2.bias"))
        return f

    def _ffn_bwd(self, b, tag, lp, df, x, site, ds_res):
        """df: grad wrt f (dropout-masked).  Returns grad wrt x (+ ds_res)."""
        M, d = x.shape
        ff = self.cfg["ff"]
        dhpre = b.get(tag + "dhpre", (M, ff), self.dt)
        ops.gemm(df, self.W(lp + "linear2.weight"), dhpre, ta=False, tb=False, act=self.cfg["activation"],
                 dact_src=b.t[tag + "hpre"], dropout=self.drop(site))
        self.dw_gemm(df, b.t[tag + "h"], self.G(lp + "linear2.weight"), bias_grad=self.G(lp + "linear2.bias"))
        dx = b.get(tag + "dxf", (M, d), self.dt)
        ops.gemm(dhpre, self.W(lp + "linear1.weight"), dx, ta=False, tb=False, addend=ds_res)
        self.dw_gemm(dhpre, x, self.G(lp + "linear1.weight"), bias_grad=self.G(lp + "linear1.bias"))
        return dx

