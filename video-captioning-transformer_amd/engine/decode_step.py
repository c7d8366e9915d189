"""Inference on the KV cache: the state of a greedy / beam / sampled decode session -- the one place where the three differ: how a
run starts, which cache a step works on, the selection stage and the generation controls in front of it -- and the four variants of
the per-token step with their eligibility tests.  `eng` is the DecoderEngine whose weights and switches a function works on."""
import struct

import torch

from .. import ops
from .params import _Buf


class DecodeState:
    """Static buffers of one greedy-decode session (B, Te, Lmax): id matrix, per-layer self-attention
    cache [B, Lmax, 3d] (packed q | k | v of every consumed token), per-layer cross-attention K/V of the memory (computed once), step temporaries
    and the hipGraphs of the per-token step (one per position; every kernel argument is baked)."""

    fused_select = True     # the selection is greedy's, which the batch-1 block step fuses into its generator launch

    def __init__(self, eng: "DecoderEngine", Bn: int, Te: int, Lmax: int, return_attn: bool = False, controls: bool = False, R: int = 1):
        d, L, dt, dev = eng.cfg["d"], eng.cfg["layers"], eng.dt, eng.dev
        self.B, self.Te, self.Lmax = Bn, Te, Lmax
        self.Bv, self.R = Bn // R, R      # R rows per video: the beams / samples of a subclass; greedy has one
        # controls: the 160-byte block {min_length, ngram, theta, inv_theta, n_banned, reserved[3], banned[32]} that vct_logit_controls
        # reads on the device (the captured graphs serve every setting); None = the step issues no controls launch at all
        self.gen_ctl = torch.zeros(40, dtype=torch.int32, device=dev) if controls else None
        # return_attn: row t-1 of layer l = the head-averaged cross-attention of the token consumed at step t (predict_video.py:63-64);
        # None = the step issues no map launch at all
        self.attn_maps = torch.zeros(Bn, L, max(Lmax - 1, 1), Te, dtype=torch.float32, device=dev) if return_attn else None
        self.ys = torch.zeros(Bn, Lmax, dtype=torch.long, device=dev)
        self.ended = torch.zeros(Bn, dtype=torch.bool, device=dev)
        self.ended_count = torch.zeros(1, dtype=torch.int32, device=dev)
        self.all_ended_at = torch.full((1,), Lmax, dtype=torch.long, device=dev)   # first t at which every row had ended
        self.kv_self = [torch.zeros(Bn * Lmax, 3 * d, dtype=dt, device=dev) for _ in range(L)]    # [q | k | v] per slot
        self.kv_cross = [torch.empty(Bn * Te, 2 * d, dtype=dt, device=dev) for _ in range(L)]
        self.mem_rep = None     # a beam / sampled session allocates it: the memory replicated per row, [B * Te, d] (also when R = 1)
        self.b = _Buf(dev, eng.ps.ctx)
        self.graphs = {}
        self.pad_id = self.last_logits = None     # last_logits: [B, Vp] of the last step, after the controls, if any
        # decode's session loop fills these on the GPU: the captured prologue's record, second stream, pinned word, event per position
        self.begin = self.poll_stream = self.poll_host = self.events = None

    def set_controls(self, controls):
        """Write the generation controls of the next run (decode.GenerationControls) into gen_ctl: one 160-byte host -> device
        copy on the current stream, no recapture."""
        if self.gen_ctl is None:
            raise ValueError("this decode session was built without generation controls")
        self.gen_ctl.copy_(torch.frombuffer(bytearray(controls.pack()), dtype=torch.int32))

    def start(self, eng, mem: torch.Tensor, start_id: int, pad_id: int):
        """Reset for a new run from this encoder memory (replicated per row first, in a session that holds a mem_rep): ids, end flags, cross-attention K/V of every layer."""
        d = eng.cfg["d"]
        if self.mem_rep is not None:
            self.mem_rep.view(self.Bv, self.R, self.Te, d).copy_(mem.reshape(self.Bv, 1, self.Te, d).expand(-1, self.R, -1, -1))
            mem = self.mem_rep
        self.pad_id = int(pad_id)
        self.ys.fill_(pad_id)
        self.ys[:, 0] = start_id
        self.ended.zero_()
        self.ended_count.zero_()
        self.all_ended_at.fill_(self.Lmax)
        for l in range(eng.cfg["layers"]):
            lp = f"decoder.layers.{l}.multihead_attn."
            ops.gemm(mem, eng.W(lp + "in_proj_weight")[d:], self.kv_cross[l], bias=eng.F(lp + "in_proj_bias")[d:])

    def cache(self, l: int, t: int) -> torch.Tensor:
        """Layer l's self-attention cache at step t, [B * Lmax, 3d]."""
        return self.kv_self[l]

    def slot(self, l: int, t: int) -> torch.Tensor:
        """Slot t-1 of layer l's self-attention cache, q | k | v of the token consumed at step t: a [B, 3d] view, row stride Lmax*3d."""
        return self.cache(l, t).view(self.B, self.Lmax, -1)[:, t - 1, :]

    def apply_controls(self, eng, logits: torch.Tensor, t: int, end_id: int):
        """Generation controls of a session that carries them: one vct_logit_controls launch edits the step's logits in place."""
        ops.logit_controls(logits, self.ys, self.ended, self.gen_ctl, t, end_id, cols=eng.V)

    def select(self, eng, logits: torch.Tensor, t: int, end_id: int):
        """Selection stage of a greedy step: arg-max into column t + sticky end flags + the first step at which every row has ended."""
        ops.greedy_select(logits, self.ys[:, t], end_id, self.ended, self.ended_count, self.all_ended_at, t, cols=eng.V)


def _finish_step(eng, st: DecodeState, logits: torch.Tensor, t: int, end_id: int):
    """The end of every step variant but the block step: publish the logits, apply the session's controls (if any), select."""
    st.last_logits = logits
    if st.gen_ctl is not None:
        st.apply_controls(eng, logits, t, end_id)
    st.select(eng, logits, t, end_id)


def _attn_map_row(eng, st: DecodeState, l: int, t: int, qc: torch.Tensor):
    """Sessions that return attention maps: one vct_attn_weights launch per layer once the cross-attention query of the consumed
    token exists (Lq = 1, keys = the cached K projection of the memory) -> row t-1 of layer l."""
    if st.attn_maps is not None:
        d = eng.cfg["d"]
        ops.attn_weights(qc, st.kv_cross[l][:, :d], st.attn_maps[:, l, t - 1:t, :], st.B, eng.cfg["nhead"], 1, st.Te)


def _decoder_decode_step(eng, st: DecodeState, t: int, end_id: int):
    """One greedy step with the KV cache: consumes token ys[:, t-1], writes ys[:, t].  Equivalent to
    CapDecoder.decode_word on ys[:, :t] + torch.max (CapDecoder.py:62-79, MMT4Caption.py:164-172): the
    keys/values of positions < t-1 are the cached projections of the same inputs."""
    d, H, L, Bn, Te, Lmax = eng.cfg["d"], eng.cfg["nhead"], eng.cfg["layers"], st.B, st.Te, st.Lmax
    b = st.b
    ws = eng.gemm_ws()      # split-K over the reduction for these M = batch GEMMs (a few output tiles, long K), reduced in-kernel
    eng.p_drop = 0.0
    pos_row = eng.pos[t - 1:t]                       # positional row of the consumed token
    x = ops.embed_fwd(st.ys[:, t - 1:t], 1, eng.F("tgt_to_emb.weight"), pos_row, b.get("x0", (Bn, d), eng.dt))
    for l in range(L):
        lp, tag = f"decoder.layers.{l}.", f"L{l}."
        sa = lp + "self_attn."
        # ONE packed projection per token: q, k, v land in slot t-1 of the cache [B, Lmax, 3d] (k, v stay there for the
        # later steps; q is read once, through the same row stride)
        cache = st.cache(l, t)
        qkv_new = st.slot(l, t)
        ops.gemm(x, eng.W(sa + "in_proj_weight"), qkv_new, bias=eng.F(sa + "in_proj_bias"), workspace=ws)
        o = b.get(tag + "o", (Bn, d), eng.dt)
        ops.attn_fwd(qkv_new[:, :d], cache[:, d:2 * d], cache[:, 2 * d:], o, Bn, H, 1, t, kv_batch_stride=Lmax * 3 * d)
        a = b.get(tag + "a", (Bn, d), eng.dt)
        ops.gemm(o, eng.W(sa + "out_proj.weight"), a, bias=eng.F(sa + "out_proj.bias"), workspace=ws)
        x1 = eng._ln_fwd(b, tag + "n1.", lp + "norm1.", a, x, None)
        ca = lp + "multihead_attn."
        qc = b.get(tag + "qc", (Bn, d), eng.dt)
        ops.gemm(x1, eng.W(ca + "in_proj_weight")[:d], qc, bias=eng.F(ca + "in_proj_bias")[:d], workspace=ws)
        oc = b.get(tag + "oc", (Bn, d), eng.dt)
        ops.attn_fwd(qc, st.kv_cross[l][:, :d], st.kv_cross[l][:, d:], oc, Bn, H, 1, Te)
        _attn_map_row(eng, st, l, t, qc)
        c = b.get(tag + "c", (Bn, d), eng.dt)
        ops.gemm(oc, eng.W(ca + "out_proj.weight"), c, bias=eng.F(ca + "out_proj.bias"), workspace=ws)
        x2 = eng._ln_fwd(b, tag + "n2.", lp + "norm2.", c, x1, None)
        h = b.get(tag + "h", (Bn, eng.cfg["ff"]), eng.dt)
        ops.gemm(x2, eng.W(lp + "linear1.weight"), h, bias=eng.F(lp + "linear1.bias"), act=eng.cfg["activation"], workspace=ws)
        f = b.get(tag + "f", (Bn, d), eng.dt)
        ops.gemm(h, eng.W(lp + "linear2.weight"), f, bias=eng.F(lp + "linear2.bias"), workspace=ws)
        x = eng._ln_fwd(b, tag + "n3.", lp + "norm3.", f, x2, None)
    y = eng._ln_fwd(b, "nf.", "decoder.norm.", x, None, None)
    logits = b.get("logits", (Bn, eng.Vp), eng.dt)
    ops.gemm(y, eng.W("generator.weight"), logits, bias=eng.F("generator.bias"), n_valid=eng.V, workspace=ws)
    # selection (greedy: arg-max into column t + sticky end flags + the first step at which every row has ended: one launch), no host sync
    _finish_step(eng, st, logits, t, end_id)


def _decoder_small_decode_ok(eng, st: DecodeState) -> bool:
    """The weight-streaming GEMV step (ops.decode_gemv): model widths that are whole 16-byte lane rows (d, ff multiples of
    512 for bf16 / 256 for fp32, <= 2048), <= 64 cached positions, and batch 1 -- measured per token at cfg-B
    (tools/decode_probe.py, graph replay): batch 1 97 us vs 114 us on the batched MFMA kernels, batch 2 135 vs 116 (every
    workgroup recomputes the attention of all (batch, head) pairs and reduces 8 x B dot products per trip), so every larger
    batch stays on the batched kernels."""
    ki = 512 if eng.dt == torch.bfloat16 else 256
    d, ff, H = eng.cfg["d"], eng.cfg["ff"], eng.cfg["nhead"]
    # the C side's limits (csrc/vct_decode.hip, vct_decode_gemv): K / ki chunks per lane in {1, 2, 4} (8: fp32 only), the
    # LayerNorm prologues hold a whole row of K = d <= 1024 in registers, head_dim a whole number of 16-byte vectors.  Any
    # other width (the shipped d = 768 in fp32: 3 chunks) takes the batched step instead of raising VCT_E_SHAPE.
    def chunks_ok(k):
        return k % ki == 0 and (k // ki in (1, 2, 4) or (k // ki == 8 and eng.dt == torch.float32))
    vec = 8 if eng.dt == torch.bfloat16 else 4
    return (eng.small_batch_decode and st.B <= 1 and chunks_ok(d) and chunks_ok(ff) and d <= 1024 and (d // H) % vec == 0
            and st.Lmax <= 64 and st.Te <= 64 and eng.dev.type == "cuda")


def _decoder_decode_step_small(eng, st: DecodeState, t: int, end_id: int):
    """The same step as _decoder_decode_step in 6 launches per layer + 2: embedding, LayerNorms and both attention cores run in the
    prologues of the matrix-vector kernels that consume them, residual adds in the epilogues of the producers; activations
    between stages are fp32 vectors (pre-norm sums s, normalised x kept for the next residual)."""
    d, H, L, B, Te, Lmax, ff = eng.cfg["d"], eng.cfg["nhead"], eng.cfg["layers"], st.B, st.Te, st.Lmax, eng.cfg["ff"]
    b = st.b
    f32 = torch.float32
    x, s, x1, x2 = (b.get(n, (B, d), f32) for n in ("sx", "ss", "sx1", "sx2"))
    s2, s3 = b.get("ss2", (B, d), f32), b.get("ss3", (B, d), f32)
    qc = b.get("sqc", (B, d), eng.dt)
    h = b.get("sh", (B, ff), f32)
    prev_norm = None
    for l in range(L):
        lp = f"decoder.layers.{l}."
        sa, ca = lp + "self_attn.", lp + "multihead_attn."
        cache = st.cache(l, t)                                           # [B * Lmax, 3d]: q | k | v of every consumed token
        slot = st.slot(l, t)
        if l == 0:      # x = Emb[ys[:, t-1]] + pos[t-1]  ->  q | k | v into slot t-1
            ops.decode_gemv(eng.W(sa + "in_proj_weight"), slot, B, bias=eng.F(sa + "in_proj_bias"), pro="embed",
                            embed=(st.ys[:, t - 1], eng.F("tgt_to_emb.weight"), eng.pos[t - 1]), out_native=True, x_out=x)
        else:           # x = norm3 of the layer below
            ops.decode_gemv(eng.W(sa + "in_proj_weight"), slot, B, bias=eng.F(sa + "in_proj_bias"), pro="ln", x_in=s3, ln1=prev_norm,
                            out_native=True, x_out=x)
        # s = x + out_proj(self-attention over the t cached positions)
        ops.decode_gemv(eng.W(sa + "out_proj.weight"), s, B, bias=eng.F(sa + "out_proj.bias"), pro="self_attn",
                        attn=(slot[:, :d], cache[:, d:2 * d], cache[:, 2 * d:], 3 * d, Lmax * 3 * d, H, t), res=x)
        # x1 = norm1(s); cross-attention query
        ops.decode_gemv(eng.W(ca + "in_proj_weight")[:d], qc, B, bias=eng.F(ca + "in_proj_bias")[:d], pro="ln", x_in=s,
                        ln1=(eng.F(lp + "norm1.weight"), eng.F(lp + "norm1.bias")), out_native=True, x_out=x1)
        kvc = st.kv_cross[l]                                               # [B * Te, 2d]
        ops.decode_gemv(eng.W(ca + "out_proj.weight"), s2, B, bias=eng.F(ca + "out_proj.bias"), pro="cross_attn",
                        attn=(qc, kvc[:, :d], kvc[:, d:], 2 * d, Te * 2 * d, H, Te), res=x1)
        _attn_map_row(eng, st, l, t, qc)           # (before the next layer overwrites the shared query vector)
        # x2 = norm2(s2); feed-forward
        ops.decode_gemv(eng.W(lp + "linear1.weight"), h, B, bias=eng.F(lp + "linear1.bias"), pro="ln", x_in=s2,
                        ln1=(eng.F(lp + "norm2.weight"), eng.F(lp + "norm2.bias")), act=eng.cfg["activation"], x_out=x2)
        ops.decode_gemv(eng.W(lp + "linear2.weight"), s3, B, bias=eng.F(lp + "linear2.bias"), pro="none", x_in=h, res=x2)
        prev_norm = (eng.F(lp + "norm3.weight"), eng.F(lp + "norm3.bias"))
    logits = b.get("slogits", (B, eng.Vp), f32)
    ops.decode_gemv(eng.W("generator.weight"), logits, B, bias=eng.F("generator.bias"), pro="ln_ln", x_in=s3, ln1=prev_norm,
                    ln2=(eng.F("decoder.norm.weight"), eng.F("decoder.norm.bias")), n_valid=eng.V)
    _finish_step(eng, st, logits, t, end_id)


def _decoder_block_decode_ok(eng, st: DecodeState) -> bool:
    """The batch-1 step with one launch per layer BLOCK (ops.decode_block): bf16, d = 512 with head_dim 64, ff <= 2048, <= 64 positions
    (vct_decode_block_supported is the authority: anything else falls through to the gemv / skinny / batched steps)."""
    d, ff, H = eng.cfg["d"], eng.cfg["ff"], eng.cfg["nhead"]
    if st.attn_maps is not None:      # the block step keeps its cross-attention query inside the kernel: the gemv / generic step takes over
        return False
    return (eng.block_decode and st.B == 1 and eng.dev.type == "cuda" and st.Lmax <= 64 and st.Te <= 64
            and ops.decode_block_supported(eng.dt, d, H, ff, min(st.Lmax, 64)))


def _decoder_decode_step_block(eng, st: DecodeState, t: int, end_id: int):
    """The step of _decoder_decode_step for ONE caption in 3 launches per layer + 1: self-attention block, cross-attention block,
    feed-forward block (each: first product + attention / activation + the second product split over the workgroups that own the
    first, as partial vectors), generator (its last workgroup also selects the token).  The partial vectors, the residual, the second product's bias and the
    LayerNorm(s) are folded by the prologue of the next launch (csrc/vct_decode_block.hip)."""
    d, H, L, Te, Lmax, ff = eng.cfg["d"], eng.cfg["nhead"], eng.cfg["layers"], st.Te, st.Lmax, eng.cfg["ff"]
    b = st.b
    f32 = torch.float32
    xa, x1, x2 = b.get("kx", (d,), f32), b.get("kx1", (d,), f32), b.get("kx2", (d,), f32)
    a_part, c_part, f_part = b.get("ka", (H, d), f32), b.get("kc", (H, d), f32), b.get("kf", (ff // 64, d), f32)
    prev = None                                   # (bias of linear2, norm3) of the layer below
    for l in range(L):
        lp = f"decoder.layers.{l}."
        sa, ca = lp + "self_attn.", lp + "multihead_attn."
        cache = st.cache(l, t)                                           # [Lmax, 3d]: q | k | v of every consumed token
        slot = cache[t - 1]
        src = (dict(embed=(st.ys[0, t - 1:t], eng.F("tgt_to_emb.weight"), eng.pos[t - 1])) if prev is None else
               dict(res=x2, res_bias=prev[0], part=f_part, ln1=prev[1]))
        ops.decode_block("self", d, w_a=eng.W(sa + "in_proj_weight"), b_a=eng.F(sa + "in_proj_bias"), slot=slot,
                         kc=cache[:, d:2 * d], vc=cache[:, 2 * d:], kv_ld=3 * d, Lk=t, w_b=eng.WT(sa + "out_proj.weight"),
                         part_out=a_part, x_out=xa, **src)
        kvc = st.kv_cross[l]                                               # [Te, 2d]
        ops.decode_block("cross", d, res=xa, res_bias=eng.F(sa + "out_proj.bias"), part=a_part,
                         ln1=(eng.F(lp + "norm1.weight"), eng.F(lp + "norm1.bias")), x_out=x1,
                         w_a=eng.W(ca + "in_proj_weight")[:d], b_a=eng.F(ca + "in_proj_bias")[:d], kc=kvc[:, :d], vc=kvc[:, d:],
                         kv_ld=2 * d, Lk=Te, w_b=eng.WT(ca + "out_proj.weight"), part_out=c_part)
        ops.decode_block("ffn", d, res=x1, res_bias=eng.F(ca + "out_proj.bias"), part=c_part,
                         ln1=(eng.F(lp + "norm2.weight"), eng.F(lp + "norm2.bias")), x_out=x2,
                         w_a=eng.W(lp + "linear1.weight"), b_a=eng.F(lp + "linear1.bias"), w_b=eng.WT(lp + "linear2.weight"),
                         ff=ff, act=eng.cfg["activation"], part_out=f_part)
        prev = (eng.F(lp + "linear2.bias"), (eng.F(lp + "norm3.weight"), eng.F(lp + "norm3.bias")))
    logits = b.get("klogits", (1, eng.Vp), f32)
    sel = b.t.get("ksel")
    if sel is None or sel.numel() < 2 * ((eng.V + 127) // 128) + 1:
        sel = b.get("ksel", (2 * ((eng.V + 127) // 128) + 1,), f32)
        sel.zero_()                               # the ticket counter: every launch leaves it at zero again
    ops.decode_block("gen", d, res=x2, res_bias=prev[0], part=f_part, ln1=prev[1],
                     ln2=(eng.F("decoder.norm.weight"), eng.F("decoder.norm.bias")), w_a=eng.W("generator.weight"),
                     b_a=eng.F("generator.bias"), V=eng.V, part_out=logits,
                     select=(sel, st.ys[0, t:t + 1], end_id, st.ended, st.ended_count, st.all_ended_at, t))
    st.last_logits = logits


def _decoder_fused_decode_ok(eng, st: DecodeState) -> bool:
    """The batched step with LayerNorms folded into the consuming projections (ops.decode_linear): bf16, up to 256 captions in
    flight, model width <= 1024 (a row's statistics come out of one pass over the MFMA fragments)."""
    d, ff = eng.cfg["d"], eng.cfg["ff"]
    return (eng.fused_decode and eng.dt == torch.bfloat16 and 2 <= st.B <= 256 and d % 32 == 0 and d <= 1024 and ff % 32 == 0
            and eng.dev.type == "cuda")


def _decoder_decode_step_fused(eng, st: DecodeState, t: int, end_id: int):
    """The same step as _decoder_decode_step in 8 launches per layer + 3 instead of 11 + 4: every projection is one skinny MFMA
    kernel (M = batch rows, K split over the waves); norm1 / norm2 / norm3 run as the prologue of the projection that consumes
    them (which also stores the normalised rows once, for the residual two launches later), the residual adds in the epilogues;
    the sums that feed a LayerNorm stay fp32."""
    d, H, L, Bn, Te, Lmax, ff = eng.cfg["d"], eng.cfg["nhead"], eng.cfg["layers"], st.B, st.Te, st.Lmax, eng.cfg["ff"]
    b = st.b
    f32 = torch.float32
    act = eng.cfg["activation"]
    xin, xres, prev_norm = None, None, None      # layer input: the embedded tokens (layer 0) or (pre-norm sum, norm3 of the layer below)
    for l in range(L):
        lp, tag = f"decoder.layers.{l}.", f"F{l}."
        sa, ca = lp + "self_attn.", lp + "multihead_attn."
        cache = st.cache(l, t)
        slot = st.slot(l, t)                                                # q | k | v of the consumed token
        xres = b.get(tag + "xn", (Bn, d), f32)
        if prev_norm is None:                    # x = Emb[ys[:, t-1]] + pos[t-1], built in the projection's prologue
            ops.decode_linear(eng.W(sa + "in_proj_weight"), slot, embed=(st.ys[:, t - 1], eng.F("tgt_to_emb.weight"), eng.pos[t - 1]),
                              x_norm=xres, bias=eng.F(sa + "in_proj_bias"))
        else:
            ops.decode_linear(eng.W(sa + "in_proj_weight"), slot, x_pre=xin, ln=prev_norm, x_norm=xres, bias=eng.F(sa + "in_proj_bias"))
        o = b.get(tag + "o", (Bn, d), eng.dt)
        ops.attn_fwd(slot[:, :d], cache[:, d:2 * d], cache[:, 2 * d:], o, Bn, H, 1, t, kv_batch_stride=Lmax * 3 * d)
        s1 = b.get(tag + "s1", (Bn, d), f32)                                # x + self-attention block
        ops.decode_linear(eng.W(sa + "out_proj.weight"), s1, x=o, bias=eng.F(sa + "out_proj.bias"), res=xres)
        x1 = b.get(tag + "x1", (Bn, d), f32)
        qc = b.get(tag + "qc", (Bn, d), eng.dt)
        ops.decode_linear(eng.W(ca + "in_proj_weight")[:d], qc, x_pre=s1, ln=(eng.F(lp + "norm1.weight"), eng.F(lp + "norm1.bias")),
                          x_norm=x1, bias=eng.F(ca + "in_proj_bias")[:d])
        oc = b.get(tag + "oc", (Bn, d), eng.dt)
        ops.attn_fwd(qc, st.kv_cross[l][:, :d], st.kv_cross[l][:, d:], oc, Bn, H, 1, Te)
        _attn_map_row(eng, st, l, t, qc)
        s2 = b.get(tag + "s2", (Bn, d), f32)
        ops.decode_linear(eng.W(ca + "out_proj.weight"), s2, x=oc, bias=eng.F(ca + "out_proj.bias"), res=x1)
        x2 = b.get(tag + "x2", (Bn, d), f32)
        h = b.get(tag + "h", (Bn, ff), eng.dt)
        ops.decode_linear(eng.W(lp + "linear1.weight"), h, x_pre=s2, ln=(eng.F(lp + "norm2.weight"), eng.F(lp + "norm2.bias")),
                          x_norm=x2, bias=eng.F(lp + "linear1.bias"), act=act)
        s3 = b.get(tag + "s3", (Bn, d), f32)
        ops.decode_linear(eng.W(lp + "linear2.weight"), s3, x=h, bias=eng.F(lp + "linear2.bias"), res=x2)
        xin, prev_norm = s3, (eng.F(lp + "norm3.weight"), eng.F(lp + "norm3.bias"))
    y = b.get("fy", (Bn, d), eng.dt)
    ops.decode_ln2(xin, prev_norm, (eng.F("decoder.norm.weight"), eng.F("decoder.norm.bias")), y)
    logits = b.get("logits", (Bn, eng.Vp), eng.dt)
    ops.gemm(y, eng.W("generator.weight"), logits, bias=eng.F("generator.bias"), n_valid=eng.V, workspace=eng.gemm_ws())
    _finish_step(eng, st, logits, t, end_id)


def decode_step_variant(eng, st: DecodeState) -> str:
    """The step variant of this session, 'block' | 'gemv' | 'fused' | 'generic': what _decoder_decode_step_any dispatches on.  The
    block step fuses its own greedy selection into the generator launch: a session with another selection stage or with
    generation controls (which run between the generator and the selection) takes the gemv / fused / generic step."""
    if st.fused_select and st.gen_ctl is None and _decoder_block_decode_ok(eng, st):
        return "block"
    if _decoder_small_decode_ok(eng, st):
        return "gemv"
    return "fused" if _decoder_fused_decode_ok(eng, st) else "generic"


def _decoder_decode_step_any(eng, st: DecodeState, t: int, end_id: int):
    """One step of any session (greedy, beam, sampled) on the variant its shape and selection stage allow."""
    step = {"block": _decoder_decode_step_block, "gemv": _decoder_decode_step_small, "fused": _decoder_decode_step_fused,
            "generic": _decoder_decode_step}[decode_step_variant(eng, st)]
    return step(eng, st, t, end_id)


class BeamDecodeState(DecodeState):
    """Static buffers of one beam-search session (B videos, K beams, Te, Lmax): the greedy session's buffers for M = B*K rows
    (row b*K + k = beam k of video b) with the self-attention cache as a PING-PONG pair [2][L, M*Lmax, 3d] (step t runs on side
    t % 2, and vct_beam_reorder gathers the slots < t of every row's parent into the other side), the memory replicated per
    beam (cross-attention K/V per row), and the beam state: scores fp32 [M], finished uint8 [M], parent rows int32 [Lmax, M]
    (row t: the parent of every slot chosen at step t; ids are back-tracked once at the end), ys = the token table (column t:
    the token appended at step t), per-step finished counters int32 [Lmax], all_ended_at = the first step after which every
    slot is finished."""

    fused_select = False

    def __init__(self, eng: "DecoderEngine", Bv: int, K: int, Te: int, Lmax: int, controls: bool = False):
        super().__init__(eng, Bv * K, Te, Lmax, controls=controls, R=K)      # (no attention maps: they would have to follow the parent back-track)
        d, L, dt, dev = eng.cfg["d"], eng.cfg["layers"], eng.dt, eng.dev
        M, self.K = Bv * K, K
        self.kv_self = None
        self.kv_layers = [torch.zeros(L, M * Lmax, 3 * d, dtype=dt, device=dev) for _ in range(2)]
        self.mem_rep = torch.empty(M * Te, d, dtype=dt, device=dev)
        self.scores = torch.zeros(M, dtype=torch.float32, device=dev)
        self.finished = torch.zeros(M, dtype=torch.uint8, device=dev)
        self.parents = torch.zeros(Lmax, M, dtype=torch.int32, device=dev)
        self.fin_count = torch.zeros(Lmax, dtype=torch.int32, device=dev)
        nws = ops.beam_select_workspace_bytes(torch.float32, Bv, K, eng.V) // 4     # fp32 logits (the gemv step's) need the most
        self.sel_ws = torch.empty(max(nws, 1), dtype=torch.float32, device=dev)

    def start(self, eng, mem: torch.Tensor, start_id: int, pad_id: int):
        """+ the beam state of step 0: slot 0 of every video scores 0, the others -inf (step 1 expands slot 0 only), nothing finished."""
        super().start(eng, mem, start_id, pad_id)
        self.scores.fill_(float("-inf"))
        self.scores.view(self.Bv, self.K)[:, 0] = 0.0
        self.finished.zero_()
        self.fin_count.zero_()

    def cache(self, l: int, t: int) -> torch.Tensor:
        """Step t runs on side t % 2 of the ping-pong pair."""
        return self.kv_layers[t % 2][l]

    def apply_controls(self, eng, logits: torch.Tensor, t: int, end_id: int):
        """On the token table and parent rows as they stand before vct_beam_select of step t."""
        ops.logit_controls(logits, self.ys, self.finished, self.gen_ctl, t, end_id, cols=eng.V, parents=self.parents, K=self.K)

    def select(self, eng, logits: torch.Tensor, t: int, end_id: int):
        """Selection stage of a beam step: top K per video (vct_beam_select), then the cache slots < t follow their parents into
        the other side of the ping-pong pair (vct_beam_reorder)."""
        ops.beam_select(logits, self.Bv, self.K, self.scores, self.finished, self.parents[t], self.ys[:, t], end_id, self.pad_id,
                        self.fin_count[t:t + 1], self.all_ended_at, t, self.sel_ws, cols=eng.V)
        ops.beam_reorder(self.kv_layers[t % 2], self.kv_layers[(t + 1) % 2], self.parents[t], self.B, self.Lmax, eng.cfg["d"], t)


class SampleDecodeState(DecodeState):
    """Static buffers of one sampled-decode session (B videos, N samples each, Te, Lmax): the greedy session's buffers for
    M = B*N rows (row b*N + n = sample n of video b) with the memory replicated per sample, as BeamDecodeState replicates it per
    beam -- but ONE self-attention cache (rows never change parents, so nothing is reordered) -- and the sampling state: ctl,
    the 16-byte control block {uint32 seed, int32 top_k, float inv_temp, float top_p} that vct_sample_select reads on the
    device (the captured graphs serve every setting), step_logp fp32 [Lmax, M] (row t: the log-probability of the token drawn
    at step t, 0 for a row that had ended), seq_logp fp32 [M] (their sum) and the selection workspace."""

    fused_select = False

    def __init__(self, eng: "DecoderEngine", Bv: int, N: int, Te: int, Lmax: int, controls: bool = False):
        super().__init__(eng, Bv * N, Te, Lmax, controls=controls, R=N)      # (no attention maps: return_attn is a greedy-decode feature)
        dev = eng.dev
        M, self.N = Bv * N, N
        self.mem_rep = torch.empty(M * Te, eng.cfg["d"], dtype=eng.dt, device=dev)
        self.ctl = torch.zeros(4, dtype=torch.int32, device=dev)
        self.step_logp = torch.zeros(Lmax, M, dtype=torch.float32, device=dev)
        self.seq_logp = torch.zeros(M, dtype=torch.float32, device=dev)
        nws = ops.sample_select_workspace_bytes(torch.float32, M, eng.V) // 4     # fp32 logits (the gemv step's) need the most
        self.sel_ws = torch.empty(max(nws, 4), dtype=torch.float32, device=dev)

    def set_sampling(self, seed: int, top_k: int, temperature: float, top_p: float):
        """Write the sampling settings of the next run into ctl (one 16-byte host -> device copy on the current stream)."""
        raw = struct.pack("<Iiff", int(seed) & 0xFFFFFFFF, int(top_k), 1.0 / float(temperature), float(top_p))
        self.ctl.copy_(torch.frombuffer(bytearray(raw), dtype=torch.int32))

    def start(self, eng, mem: torch.Tensor, start_id: int, pad_id: int):
        """+ the log-probabilities (ctl is the caller's: it is written before the replays, not by the captured begin graph)."""
        super().start(eng, mem, start_id, pad_id)
        self.step_logp.zero_()
        self.seq_logp.zero_()

    def select(self, eng, logits: torch.Tensor, t: int, end_id: int):
        """Selection stage of a sampled step: one draw per row (vct_sample_select) into column t, its log-probability into row t
        of step_logp and onto seq_logp, greedy's end bookkeeping."""
        ops.sample_select(logits, self.ys[:, t], end_id, self.pad_id, self.ended, self.ended_count, self.all_ended_at, t,
                          self.step_logp[t], self.seq_logp, self.ctl, self.sel_ws, cols=eng.V)
