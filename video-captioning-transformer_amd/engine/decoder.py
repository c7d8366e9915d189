"""Forward / backward schedule of the caption decoder (training) and its decode entry points."""
import os
from typing import Optional

import torch

from .. import ops
from . import decode_step as _ds
from .stack import DEC_SITE, DMEM_SYNC, EMB_SITE, _StackBase


class DecoderEngine(_StackBase):
    """CapDecoder: embedding + positional table, decoder stack, generator, SCE loss
    (model/CapDecoder.py:34-60)."""

    # A/B switch: vocabulary dX through a transposed weight shadow (NT form on the persistent 256x256 kernel, split over K).  The shadow is
    # maintained by the parameter set (ParamSet.want_transposed): one 35 us transpose behind the optimizer's pass over W_g, in the main
    # stream's slack at the end of the step.  (Rebuilt in front of the layer stack at every step it cost the forward more than the dX
    # gained.)  Measured in the step (same box): the dX bracket drops 0.218 -> 0.181 ms and the Adam bracket grows by the 40 us of the
    # transpose; step 2.44-2.45 ms either way (the chip is work-bound: the side stream fills whatever the main stream leaves) -> off.
    # (round 6: the NN form on the pipelined 256x256 kernel runs at the NT form's speed -- 0.183 ms both -- so the transposed shadow W_g^T
    # (a 39 us transpose + the 2-D optimizer pass per step behind a gradient exchange) is no longer kept by default: exchange path -0.8 %)
    gen_dx_nt = os.environ.get("VCT_GEN_DX_NT", "0") != "0"
    early_gen_dw = os.environ.get("VCT_GEN_DW_EARLY", "0") == "1"
    # bit 0 / bit 1: the bottom decoder layer's cross-attention + feed-forward / self-attention weight gradients on the MAIN stream (A/B)
    l0_dw_main = int(os.environ.get("VCT_L0_DW_MAIN", "3"))
    fused_decode = True             # A/B switch: LayerNorms folded into the skinny projections (2 <= batch <= 256, bf16)
    block_decode = os.environ.get("VCT_BLOCK_DECODE", "1") != "0"   # A/B switch: 3 launches per layer at batch 1 (bf16)
    small_batch_decode = True       # A/B switch: weight-streaming GEMV step for batch <= 4
    attn_maps = False               # set per ENGINE by CapDecoder(custom_decoder_type=...): every forward also leaves the cross-attention maps
    loss_stats = False              # set per ENGINE by CapDecoder.loss_stats: the caption loss also leaves (NLL, token accuracy) at label_smoothing 0

    def __init__(self, ps, prefix, cfg, seed, pos_buffer: torch.Tensor):
        super().__init__(ps, prefix, cfg, seed)
        self.pos = pos_buffer  # [5000, d] fp32 buffer
        self.V = cfg["vocab"]
        self.Vp = (self.V + 31) // 32 * 32
        # set per ENGINE by trainer.CaptionTrainer (single GPU, fused optimizer): nothing but this engine's backward schedule writes
        # the flat gradient buffer, so the token-embedding gradient only re-zeroes the rows it wrote in the previous step
        self.exclusive_grads = False
        ls = range(cfg["layers"])      # per layer: parameter prefix, buffer tag, dropout site base (lists for _stack_ss; the unfused loops index them)
        self.lps, self.tags, self.sites = [f"decoder.layers.{l}." for l in ls], [f"L{l}." for l in ls], [DEC_SITE + 16 * l for l in ls]
        self._wgt = None     # W_g^T of the current forward when the vocabulary dX runs in its NT form (gen_dx_nt), else None
        self.last_attn_maps = None     # attn_maps: fp32 [B, S-1, Te] per layer of the last forward (views of static buffers)
        self.last_loss_stats = None    # fp32 [2] (un-smoothed NLL, token accuracy) of the last forward that ran ops.sce_loss_ls, else None

    def _ws_grew(self):
        self.ps.ctx.generation += 1      # recordings that baked the outgrown id workspace are dropped by their owners

    def _embed(self, b, ids, Sd, M):
        return ops.embed_fwd(ids, Sd, self.F("tgt_to_emb.weight"), self.pos, b.get("x0", (M, self.cfg["d"]), self.dt),
                             dropout=self.drop(EMB_SITE))

    def _self_block(self, b, l, x, Bn, Sd, kpm):
        """x1 = LN1(x + drop(SelfMHA(x))) of decoder layer l."""
        lp, tag, site = self.lps[l], self.tags[l], self.sites[l]
        b.t[tag + "x"] = x
        return self._attn_ln_fwd(b, tag + "sa.", tag + "n1.", lp + "self_attn.", lp + "norm1.", x, x, Bn, Sd, Sd, True, kpm,
                                 site + 1, site + 2)

    def forward_prefix(self, Bn: int, Te: int, ids: torch.Tensor, training: bool):
        """The part of the decoder forward that does not depend on the encoder memory -- token embedding and the bottom
        layer's self-attention block -- issued on the side stream so that it runs beside the encoder forward
        (MMT4Caption._forward_loss calls this BEFORE the encoder is enqueued; forward() picks the result up)."""
        pad, S = self.cfg["pad_id"], ids.shape[1]
        Sd, M = S - 1, Bn * (S - 1)
        self.p_drop = self.cfg["dropout"] if training else 0.0
        if self._ss_ok(Sd, Te, Bn):     # one workgroup per sample fills every CU: nothing to run beside the encoder
            self._prefix = None
            return
        b = self.buf((Bn, Te, S))
        kpm = ("ids", ids, pad)

        def run(_ws):
            x = self._embed(b, ids, Sd, M)
            return x, self._self_block(b, 0, x, Bn, Sd, kpm)
        x, x1 = self._on_side(run)
        self._prefix = (b, x, x1)

    def _run_stack(self, b, mem, Bn, Te, ids, Sd, kpm):
        """Embedding + decoder layers + final LayerNorm over the first Sd tokens of each ids row."""
        d, L = self.cfg["d"], self.cfg["layers"]
        M = Bn * Sd
        prefix, self._prefix = self._prefix, None
        if self._ss_ok(Sd, Te, Bn) and prefix is None:
            self._kv_prefetched, self._kv_inplace = None, set()
            x0 = b.get("x0", (M, d), self.dt)                              # built by the kernel's prologue (token embedding + positions + dropout)
            x, y = self._stack_ss(b, self.lps, self.tags, x0, Bn, Sd, self.sites, ln_tag="n3.", ln_name="norm3.", final="decoder.norm.",
                                  mem=mem, Lm=Te, causal=True, kpm=kpm,
                                  embed=(ids, self.F("tgt_to_emb.weight"), self.pos, EMB_SITE))
            b.t["x_last"] = x
            return y
        if prefix is not None and prefix[0] is b:        # embedding + bottom self-attention already ran beside the encoder
            x, x1_0 = prefix[1], prefix[2]
            # the main stream has nothing else to do until the bottom cross-attention: its K/V projection runs here, in
            # place (no cross-stream hand-over on the critical path); the upper layers' go to the side stream
            self.join_side()
            self.prefetch_cross_kv(b, mem, [(f"L{l}.ca.", f"decoder.layers.{l}.multihead_attn.") for l in range(1, L)])
            self._kv_inplace = {"L0.ca."}
        else:
            self.prefetch_cross_kv(b, mem, [(f"L{l}.ca.", f"decoder.layers.{l}.multihead_attn.") for l in range(L)])
            self._kv_inplace = set()
            x, x1_0 = self._embed(b, ids, Sd, M), None
        for l in range(L):
            lp, tag, site = self.lps[l], self.tags[l], self.sites[l]
            if l == 0 and x1_0 is not None:
                x1 = x1_0
            else:
                x1 = self._self_block(b, l, x, Bn, Sd, kpm)
            x2 = self._attn_ln_fwd(b, tag + "ca.", tag + "n2.", lp + "multihead_attn.", lp + "norm2.", x1, mem, Bn, Sd, Te, False, None,
                                   site + 3, site + 4, self_attn=False)
            f = self._ffn_fwd(b, tag + "ff.", lp, x2, site + 5)
            if l == L - 1:       # norm3 of the last layer + the stack-final norm: one launch
                x, y = self._ln_ln_fwd(b, tag + "n3.", lp + "norm3.", f, x2, site + 6, "nf.", "decoder.norm.")
                self._kv_prefetched = None
                b.t["x_last"] = x
                return y
            x = self._ln_fwd(b, tag + "n3.", lp + "norm3.", f, x2, site + 6)
        self._kv_prefetched = None
        b.t["x_last"] = x
        return self._ln_fwd(b, "nf.", "decoder.norm.", x, None, None)

    def forward(self, mem: torch.Tensor, Bn: int, Te: int, ids: torch.Tensor, training: bool, want_logits=False,
                seq_w: Optional[torch.Tensor] = None, score: bool = False):
        """mem [B*Te, d] compute dtype; ids int64 [B,S] (pads = pad_id).  Returns (loss[1] fp32, logits or None).
        The logits gradient is produced in the same pass (in place when logits are not requested).

        seq_w (fp32 [B] on the device, one weight per id row): the self-critical policy-gradient loss
        -(sum over non-pad tokens of seq_w[row] * log p(token)) / (number of non-pad tokens) with its logits gradient
        (ops.wce_loss) in place of the SCE loss.  The RCE term and sce_loss_alpha are IGNORED on this path: the policy gradient of
        an expected reward is -A * grad log p and nothing else.  score=True: forward only (no logits gradient is written; backward()
        must not follow), unit weights.  Both leave the per-token log-probabilities fp32 [B*(S-1)] (0 on pad rows) in the
        buffer set as "tok_logp".

        cfg["label_smoothing"] = eps > 0 (or loss_stats at eps = 0): the SCE loss with its CE term smoothed (ops.sce_loss_ls), which
        also leaves (un-smoothed NLL, token accuracy) fp32 [2] in the buffer set as "loss_stats" -- a recorded launch list or a
        captured graph rewrites it on every replay.  eps is a launch scalar like sce_loss_alpha: a recording keeps the value it was
        made with.  With neither, the call is the ops.sce_loss call it always was.  The seq_w / score paths (ops.wce_loss) IGNORE
        eps as they ignore sce_loss_alpha: a policy gradient is not regularised towards the uniform distribution."""
        pad = self.cfg["pad_id"]
        S = ids.shape[1]
        Sd, M = S - 1, Bn * (S - 1)
        self.p_drop = self.cfg["dropout"] if training else 0.0
        b = self.buf((Bn, Te, S))
        self.cur, self.shape = b, (Bn, Te, S)
        b.t["ids"], b.t["mem"] = ids, mem
        kpm = ("ids", ids, pad)          # tgt_padding_mask[:, :-1] == (ids[:, :Sd] == pad), evaluated inside the attention kernel
        b.t["kpm"] = kpm
        self._wgt = None
        if training and self.gen_dx_nt and self.dt == torch.bfloat16 and self.dev.type == "cuda" and self.ps.dw_adam is None:
            # (Not with the optimizer inside the vocabulary weight-gradient GEMM: an epilogue that also emitted W_g^T -- per-wave LDS
            # transposition, 16-byte pieces of the transposed rows -- took that product from 328 to 413 us for a dX that is 40 us
            # faster in the NT form; round 5, gpurun_out/r5f.  dX then runs in its NN form.)
            # dX = dlogits W_g in the K-contiguous NT form (persistent 256x256 kernel, split over K): needs W_g^T, which the
            # parameter set keeps beside the bf16 shadow -- rewritten right after the optimizer has touched W_g (62 MB of traffic
            # in the main stream's slack at the end of the step), not here in front of the latency-bound layer stack
            self._wgt = self.ps.want_transposed(self.pre + "generator.weight", eager=True)
        y = self._run_stack(b, mem, Bn, Te, ids, Sd, kpm)
        ops.tap("layers_fwd", 1)
        logits = b.get("logits", (M, self.Vp), self.dt)
        ops.gemm(y, self.W("generator.weight"), logits, bias=self.F("generator.bias"), n_valid=self.V, tag="gen_fwd")
        loss = b.get("loss", (1,), torch.float32)
        dlogits = None if score else (b.get("dlogits", (M, self.Vp), self.dt) if want_logits else logits)
        ops.tap("loss", 0)
        eps = float(self.cfg.get("label_smoothing", 0.0))
        self.last_loss_stats = None
        if seq_w is not None or score:
            ops.wce_loss(logits, self.V, ids[:, 1:], Sd, pad, seq_w, loss, dlogits, b.get("row_ws", (2 * M + 2,), torch.float32),
                         tok_logp=b.get("tok_logp", (M,), torch.float32))
        elif eps > 0.0 or self.loss_stats:
            stats = self.last_loss_stats = b.get("loss_stats", (2,), torch.float32)
            ops.sce_loss_ls(logits, self.V, ids[:, 1:], Sd, pad, self.cfg["sce_loss_alpha"], eps, loss, dlogits,
                            b.get("row_ws_ls", (4 * M + 2,), torch.float32), stats=stats)
        else:
            ops.sce_loss(logits, self.V, ids[:, 1:], Sd, pad, self.cfg["sce_loss_alpha"], loss, dlogits,
                         b.get("row_ws", (2 * M + 2,), torch.float32))
        ops.tap("loss", 1)
        b.t["dlogits_used"] = dlogits
        if self.attn_maps:
            self.last_attn_maps = self._cross_attn_maps(b, Bn, Sd, Te)
        return loss, (logits if want_logits else None)

    def _cross_attn_maps(self, b, Bn, Sd, Te):
        """The head-averaged cross-attention probabilities of every layer, from the query and K projections the forward saved (the
        sample-stationary stack's cq / ckv, the unfused schedule's ca. buffers): one vct_attn_weights launch per layer behind the loss,
        nothing recomputed but the scores.  In training these are the probabilities BEFORE dropout."""
        d, H = self.cfg["d"], self.cfg["nhead"]
        maps = []
        for tag in self.tags:
            w = b.get(tag + "ca.w", (Bn, Sd, Te), torch.float32)
            maps.append(ops.attn_weights(b.t[tag + "ca.q"], b.t[tag + "ca.kv"][:, :d], w, Bn, H, Sd, Te))
        return maps

    def decode_word(self, mem: torch.Tensor, Bn: int, Te: int, ys: torch.Tensor) -> torch.Tensor:
        """Reference algorithm of CapDecoder.decode_word (CapDecoder.py:62-79): re-run the decoder over
        ALL t tokens so far (causal mask, no padding mask), generator on the last position -> [B, V]."""
        d, t = self.cfg["d"], ys.shape[1]
        self.p_drop = 0.0
        b = self.buf(("decode", Bn, Te, t))
        y = self._run_stack(b, mem, Bn, Te, ys, t, None)
        last = y.view(Bn, t, d)[:, t - 1, :]           # strided [B, d] view (lda = t*d): no gather copy
        logits = b.get("logits1", (Bn, self.Vp), self.dt)
        ops.gemm(last, self.W("generator.weight"), logits, bias=self.F("generator.bias"), n_valid=self.V)
        return logits[:, :self.V]

    # ---- inference on the KV cache, for every kind of session: the state and the step variants are in decode_step.py ----
    def decode_begin(self, st, mem, start_id, pad_id): return st.start(self, mem, start_id, pad_id)
    def decode_step(self, st, t, end_id): return _ds._decoder_decode_step_any(self, st, t, end_id)

    def backward(self, bucket_ready=None, on_dmem_ready=None, join: bool = True) -> torch.Tensor:
        """d(loss) = 1.  Returns d(memory) [B*Te, d].  bucket_ready(kind, layer) is called when a gradient bucket
        of MMT4Caption.grad_buckets() is complete ('generator', 'dec_layer' l, 'embedding').  on_dmem_ready(dmem) is
        called as soon as the last cross-attention backward has been enqueued -- d(memory) is final there, while the
        bottom layer's self-attention backward and the embedding gradient are still to come."""
        b = self.cur
        Bn, Te, S = self.shape
        d, L, pad = self.cfg["d"], self.cfg["layers"], self.cfg["pad_id"]
        Sd, M = S - 1, Bn * (S - 1)
        mem, ids, kpm = b.t["mem"], b.t["ids"], b.t["kpm"]
        dl, y = b.t["dlogits_used"], b.t["nf.y"]
        dy = b.get("dy", (M, d), self.dt)
        if self._wgt is not None:
            # fp32 partials of the split over the vocabulary-long K: room for the 6-way split of cfg-B / the 5-way one at batch 1024
            ws = b.get("gen_dx_ws", (6 * dy.shape[0] * dy.shape[1],), torch.float32)
            ops.gemm(dl, self._wgt, dy, ta=False, tb=True, k_valid=self.V, workspace=ws, tag="gen_dx")
        else:
            ops.gemm(dl, self.W("generator.weight"), dy, ta=False, tb=False, k_valid=self.V, workspace=self.gemm_ws(), tag="gen_dx")
        # the vocabulary weight gradient: with a gradient exchange it goes out first (its bucket is a third of the bytes and
        # can be on the wire during the whole backward); without one and with the encoder backward on the side stream it
        # is DEFERRED to the end of the main stream's tail, where that stream would otherwise idle -- beside the decoder's
        # dX chain it slowed the critical path (a 34 us GEMM took 123 us next to it)
        defer_gen_dw = self.defer_gen_dw and bucket_ready is None and on_dmem_ready is not None
        early_gen_dw = self.early_gen_dw and bucket_ready is None and on_dmem_ready is not None
        if early_gen_dw:      # A/B: right behind the dX GEMM on the main stream, alone on the chip (nothing runs on the side stream yet)
            defer_gen_dw = False
            ops.gemm(dl, y, self.G("generator.weight"), ta=True, tb=False, bias_grad=self.G("generator.bias"), m_valid=self.V,
                     tag="gen_dw", workspace=self.gemm_ws(), adam=self.dw_adam_desc(dl, self.G("generator.weight")))

        def gen_dw():
            if early_gen_dw:
                return
            if defer_gen_dw:
                # (Measured and dropped, round 5: this product at ONE workgroup per CU -- 40 KB of idle dynamic LDS -- so that the encoder
                # backward's short kernels on the side stream find free registers beside it: the product went 320 -> 426 us and the
                # step 2.254 -> 2.289 ms.)
                ops.gemm(dl, y, self.G("generator.weight"), ta=True, tb=False, bias_grad=self.G("generator.bias"), m_valid=self.V,
                         tag="gen_dw", workspace=self.gemm_ws(), adam=self.dw_adam_desc(dl, self.G("generator.weight")))
            else:
                self.dw_gemm(dl, y, self.G("generator.weight"), bias_grad=self.G("generator.bias"), m_valid=self.V, tag="gen_dw")
        if not defer_gen_dw:
            gen_dw()
        if bucket_ready is not None:
            self.bucket_on_side(bucket_ready, "generator")
        if not self.fuse_ln_ln_bwd:
            dx, _ = self._ln_bwd(b, "nf.", "decoder.norm.", dy, b.t["x_last"], None, None)
        dmem = b.get("dmem", (Bn * Te, d), self.dt)
        for l in reversed(range(L)):
            lp, tag, site = self.lps[l], self.tags[l], self.sites[l]
            x, x1, x2 = b.t[tag + "x"], b.t[tag + "n1.y"], b.t[tag + "n2.y"]
            if l == L - 1 and self.fuse_ln_ln_bwd:      # stack-final norm + this layer's norm3: one launch
                ds3, df = self._ln_ln_bwd(b, "nf.", "decoder.norm.", dy, b.t["x_last"], tag + "n3.", lp + "norm3.", b.t[tag + "ff.f"], x2,
                                          site + 6)
            else:
                ds3, df = self._ln_bwd(b, tag + "n3.", lp + "norm3.", dx, b.t[tag + "ff.f"], x2, site + 6)
            dx2 = self._ffn_bwd(b, tag + "ff.", lp, df, x2, site + 5, ds3)
            ds2, dc = self._ln_bwd(b, tag + "n2.", lp + "norm2.", dx2, b.t[tag + "ca.a"], x1, site + 4)
            dx1 = self._attn_block_bwd(b, tag + "ca.", lp + "multihead_attn.", dc, x1, mem, Bn, Sd, Te, False, None, site + 3,
                                       False, ds2, dkv_out=dmem, dkv_accumulate=(l != L - 1))
            dmem_point = None
            if l == 0 and on_dmem_ready is not None:
                # d(memory) is final once everything enqueued so far has run: remember that point; the encoder backward is
                # ENQUEUED after this layer's short tail (the host needs ~0.3 ms to launch its ~35 kernels, during which the
                # main stream would starve) but only WAITS for this point
                dmem_point = DMEM_SYNC
                ops.sync_record(dmem_point)
                # the bottom layer's weight gradients run on the MAIN stream (whose tail is not the critical path any
                # more): the side stream is free for the encoder backward the moment d(memory) is final
                # (With the optimizer inside the weight-gradient GEMMs this group REWRITES the layer's weights, W_kv among them, which
                # the layer's d(memory) product -- queued on the SIDE stream -- reads: the group then waits for the end of the layer's
                # chain, where the main stream first joins the side stream; tests/test_executor_gpu.py delays the side stream to show it.)
                if self.ps.dw_adam is None:
                    self.flush_dw(main=self.l0_dw_main & 1 != 0)
            ds1, da = self._ln_bwd(b, tag + "n1.", lp + "norm1.", dx1, b.t[tag + "sa.a"], x, site + 2)
            dx = self._attn_block_bwd(b, tag + "sa.", lp + "self_attn.", da, x, x, Bn, Sd, Sd, True, kpm, site + 1, True, ds1)
            if l == 0 and on_dmem_ready is not None:
                if self.ps.dw_adam is not None and self.side is not None and self.overlap_dw and self.l0_dw_main:
                    ops.stream_wait(None, self.side)          # the d(memory) products are behind us: one group of seven on the main stream
                    self.flush_dw(main=True)
                else:
                    self.flush_dw(main=self.l0_dw_main & 2 != 0)
                if bucket_ready is not None:
                    self.flush_ln_grads(b)
                    # through the side stream like every other bucket: the hook's optimizer step REWRITES this layer's weights (and
                    # their bf16 shadow), which the layer's d(memory) GEMM -- still queued on the side stream -- reads.  Handing the
                    # bucket over from the main stream alone let Adam overtake that GEMM (found by the four-rank one-GPU test: wrong
                    # encoder gradients / parameter updates on boxes where the side stream lagged)
                    self.bucket_on_side(bucket_ready, "dec_layer", l)
                self.flush_ln_grads(b)
                ops.embed_bwd(ids, Sd, pad, dx, self.G("tgt_to_emb.weight"), dropout=self.drop(EMB_SITE),
                              exclusive=self.exclusive_grads and bucket_ready is None, on_grow=self._ws_grew)
                if bucket_ready is not None:
                    bucket_ready("embedding")
                if defer_gen_dw:
                    gen_dw()
                on_dmem_ready(dmem, dmem_point)           # the encoder backward goes to the side stream now
                if join:
                    self.join_side()
                return dmem
            self.flush_dw()               # this layer's weight gradients: one grouped launch beside the next layer
            if bucket_ready is not None:      # this layer's (and, for the top layer, the final norm's) gradients are complete
                self.flush_ln_grads(b)
                self.bucket_on_side(bucket_ready, "dec_layer", l)
        self.flush_ln_grads(b)
        ops.embed_bwd(ids, Sd, pad, dx, self.G("tgt_to_emb.weight"), dropout=self.drop(EMB_SITE),
                      exclusive=self.exclusive_grads and bucket_ready is None, on_grow=self._ws_grew)
        if bucket_ready is not None:
            bucket_ready("embedding")
        if join:
            self.join_side()
        return dmem

