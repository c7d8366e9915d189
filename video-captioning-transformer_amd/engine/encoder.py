"""Forward / backward schedule of the multi-modal video encoder."""
import os

import torch

from .. import ops
from .stack import ENC_IN_SITE, ENC_SITE, _StackBase


class EncoderEngine(_StackBase):
    """MultiModalEncoder: model/MMEncoder.py:12-48, 83-104, 244-276.  The shipped combination ('avg' aggregation token, sinusoidal
    temporal encoding, no input norm; one modality, or n >= 2 with the modal embedding) runs on its own front-end kernels; any other
    combination of cfg's global_type ('avg' | 'max'), temporal_type ('encoding' | 'embedding') and do_norm (MMEncoder.py:118-197,
    240-242) goes through vct_enc_frontend_ex_* (_forward_streams(ex=True))."""

    # A/B switch: 1 = a side-stream backward puts the upper layers' weight-gradient groups behind the main stream's tail, 2 = all, 0 = none
    enc_dw_main = int(os.environ.get("VCT_ENC_DW_MAIN", "1"))

    def __init__(self, ps, prefix, cfg, seed, pe_buffer: torch.Tensor):
        super().__init__(ps, prefix, cfg, seed)
        self.pe = pe_buffer  # [1, 512, d] fp32 buffer `temp_emb.pe` (None with the learned temporal embedding)
        self._pe_rows = {}
        self._mm_rows = {}
        self._ex_rows = {}
        self.learned, self.by_max, self.do_norm = (cfg.get("temporal_type", "encoding") == "embedding", cfg.get("global_type", "avg") == "max",
                                                   bool(cfg.get("do_norm", False)))
        self.variant = self.learned or self.by_max or self.do_norm      # anything but the shipped combination
        self.mm_Ts = None    # frame counts of the modalities of the current shape (None: one modality)
        ls = range(cfg["layers"])      # per layer: parameter prefix, buffer tag, dropout site base (lists for _stack_ss; the unfused loops index them)
        self.lps, self.tags, self.sites = [f"transformer_encoder.layers.{l}." for l in ls], [f"L{l}." for l in ls], [ENC_SITE + 16 * l for l in ls]
        self.main_stream = None     # the step's own stream while backward() runs on the side stream (MMT4Caption._backward sets it around the call)

    def _mask_u8(self, mask):
        """A frame mask as the kernels read it: contiguous, bool viewed as uint8."""
        mk = mask if mask.is_contiguous() else mask.contiguous()
        return mk.view(torch.uint8) if mk.dtype == torch.bool else mk

    def _cast_in(self, b, name, x_in):
        """x_in in the compute dtype: its cast into the buffer `name` (fp32 features: the reference contract), or itself (a DeviceLoader's bf16)."""
        return x_in if x_in.dtype == self.dt else ops.cast(x_in, b.get(name, tuple(x_in.shape), self.dt))

    def pe_rows(self, T):
        r = self._pe_rows.get(T)
        if r is None:
            import numpy as np
            idx = torch.from_numpy(np.linspace(0, T - 1, T).astype(np.int64)).to(self.dev)  # MMEncoder.py:98
            r = torch.zeros(T + 1, self.cfg["d"], dtype=torch.float32, device=self.dev)
            r[1:] = self.pe[0, idx, :]
            self._pe_rows[T] = r
        return r

    @staticmethod
    def temporal_index(Ts):
        """Rows of temp_emb.embedding.weight the memory rows read (TemporalEmbedding, MMEncoder.py:150-158): 0 on every aggregation
        row, np.linspace(1, T_0, T_i) as int32 on the frames of stream i."""
        import numpy as np
        return np.concatenate([np.concatenate([np.zeros(1, np.int32), np.linspace(1, Ts[0], t).astype(np.int32)]) for t in Ts])

    def ex_rows(self, Ts):
        """The per-shape tables of vct_enc_frontend_ex_*, built once per frame-count tuple: dict(temp | tidx, labels)."""
        r = self._ex_rows.get(Ts)
        if r is None:
            n = len(Ts)
            r = {"labels": None}
            if self.learned:
                idx = self.temporal_index(Ts)
                rows = self.F("temp_emb.embedding.weight").shape[0]
                if int(idx.max()) >= rows:
                    raise ValueError(f"temporal embedding: {Ts[0]} frames in the first stream need row {int(idx.max())} of a table of {rows}")
                r["tidx"] = torch.from_numpy(idx).to(self.dev)
            if not self.learned:      # the fixed table (and, with several streams, the labels) are the shipped paths' own
                r["temp"], r["labels"] = self.mm_rows(Ts) if n > 1 else (self.pe_rows(Ts[0]), None)
            elif n > 1:
                r["labels"] = self._mm_labels(Ts)
            self._ex_rows[Ts] = r
        return r

    def _mm_labels(self, Ts):
        n, diff = len(Ts), self.cfg.get("modal_different", True)
        labels = []
        for i, t in enumerate(Ts):
            labels += [i + n if diff else i] + [i] * t
        rows = self.F("modal_emb.modal_emb.weight").shape[0]
        if sorted(set(labels)) != list(range(rows)):
            raise ValueError(f"modal-embedding labels {sorted(set(labels))} do not cover the {rows} rows of modal_emb exactly "
                             f"(n = {n}, modal_different = {diff})")
        return torch.tensor(labels, dtype=torch.int32).to(self.dev)

    def mm_rows(self, Ts):
        """(temporal rows fp32 [S, d], row labels int32 [S]) of the multi-modal front end for the frame counts Ts, cached per Ts.
        Row t of modality i gets pe[idx_i[t]], idx_i = linspace(0, T_0 - 1, T_i) as int32 (MMEncoder.py:89-104), its aggregation
        row 0; labels: i on frame rows, i + n (modal_different) or i on the aggregation row (MMEncoder.py:35-46)."""
        r = self._mm_rows.get(Ts)
        if r is None:
            import numpy as np
            d = self.cfg["d"]
            temp = torch.zeros(sum(t + 1 for t in Ts), d, dtype=torch.float32, device=self.dev)
            at = 0
            for i, t in enumerate(Ts):
                idx = torch.from_numpy(np.linspace(0, Ts[0] - 1, t).astype(np.int32).astype(np.int64)).to(self.dev)
                temp[at + 1:at + 1 + t] = self.pe[0, idx, :]
                at += t + 1
            # the kernels take the table as given (a row with an out-of-range label gets no modal row and no gradient): _mm_labels checks
            # it here, once per shape, against the embedding it indexes -- every row of the table must be used, and nothing else
            r = self._mm_rows[Ts] = (temp, self._mm_labels(Ts))
        return r

    def forward(self, feats, mask, training: bool) -> torch.Tensor:
        """feats [B,T,Ein] fp32, mask [B,T] bool (True = padded) or None -> memory [B*(T+1), d].  A list of n >= 2 modalities
        (feats [B,T_i,E_i], masks [B,T_i] or None) -> memory [B*S, d], S = sum_i (T_i + 1)."""
        n = self.cfg.get("n_modal", 1)
        got = len(feats) if isinstance(feats, (list, tuple)) else 1
        if got != n:        # (a stream short would leave its unify / modal-embedding gradients unwritten: stale ones get stepped)
            raise ValueError(f"the encoder has {n} feature stream(s), got {got}" + (" (a bare tensor)" if n > 1 and got == 1 else ""))
        if self.variant:
            many = isinstance(feats, (list, tuple))
            return self._forward_streams(list(feats) if many else [feats], (list(mask) if many else [mask]) if mask is not None else None,
                                         training, ex=True)
        if isinstance(feats, (list, tuple)):
            if n > 1:
                return self._forward_streams(feats, mask, training)
            feats, mask = feats[0], (mask[0] if mask is not None else None)
        self.mm_Ts = None
        B, T, Ein = feats.shape
        d = self.cfg["d"]
        self.p_drop = self.cfg["dropout"] if training else 0.0
        b = self.buf((B, T))
        self.cur, self.shape = b, (B, T)
        Te, M = T + 1, B * (T + 1)
        x_in = feats.reshape(B * T, Ein).contiguous()
        # key-padding of the encoder's self-attention: the raw frame mask with a shift of one (key 0 = the aggregation
        # token, never padded) -- read by the attention kernel directly, no [B, T+1] mask is built
        kpm = (self._mask_u8(mask), 1) if mask is not None else None
        b.t["kpm_used"] = kpm
        if self._ss_ok(Te, 0, B) and Ein == d and x_in.dtype in (torch.float32, self.dt):
            # the whole stack in one launch per four layers: front end (unify Linear, mean token, temporal encoding) in the kernel's
            # prologue, the stack-final norm in its last epilogue
            xc = None
            if x_in.dtype != self.dt:
                xc = b.get("feats_c", (B * T, Ein), self.dt)            # bf16 copy of the features: the unify weight gradient's operand
            b.t["x_in"] = xc if xc is not None else x_in
            x0 = b.get("x0", (M, d), self.dt)
            x, mem = self._stack_ss(b, self.lps, self.tags, x0, B, Te, self.sites, ln_tag="n2.", ln_name="norm2.",
                                    final="transformer_encoder.norm.", kpm=kpm,
                                    frontend=(x_in, xc, self.F("unify.0.bias"), self.pe_rows(T)))
            b.t["x_last"] = x
            return mem
        x_in = b.t["x_in"] = self._cast_in(b, "feats_c", x_in)
        u = b.get("u", (B * T, d), self.dt)
        ops.gemm(x_in, self.W("unify.0.weight"), u, bias=self.F("unify.0.bias"))
        x = ops.enc_frontend_fwd(u, self.pe_rows(T), b.get("x0", (M, d), self.dt), B, T)
        return self._stack_fwd(b, x, B, Te, kpm)      # (features of another width: the front end stays on its own kernels)

    def _forward_streams(self, feats, masks, training: bool, ex: bool = False) -> torch.Tensor:
        """A list of feature streams: per-stream input cast and unify GEMM, ONE front-end launch, then the stack (MMEncoder.py:244-274).
        ex = False (the shipped combination, n >= 2): vct_mm_frontend_fwd -- aggregation rows, temporal rows, modal embedding, the
        [B, S] key padding.  ex = True (any other combination, n >= 1): vct_enc_frontend_ex_fwd -- aggregation by mean or max, fixed or
        learned temporal rows, modal embedding, Dropout(LayerNorm(.)), key padding."""
        B = feats[0].shape[0]
        Ts = tuple(int(f.shape[1]) for f in feats)
        d = self.cfg["d"]
        S = sum(t + 1 for t in Ts)
        if any(f.shape[0] != B for f in feats) or (masks is not None and len(masks) != len(feats)):
            raise ValueError("multi-modal encoder: every modality needs the same batch and one mask (or masks=None)")
        if S > 64:      # (vct_attn_*: Lq, Lk <= 64 -- the encoder's self-attention and the decoder's cross-attention)
            raise ValueError(f"multi-modal encoder: {S} memory rows (sum of T_i + 1 over the streams {Ts}); the attention kernels "
                             "take at most 64")
        self.p_drop = self.cfg["dropout"] if training else 0.0
        b = self.buf((B, Ts))
        self.cur, self.shape, self.mm_Ts = b, (B, S - 1), Ts
        us = []
        for i, f in enumerate(feats):
            E = f.shape[2]
            x_in = f.reshape(B * Ts[i], E)
            if not x_in.is_contiguous():
                x_in = x_in.contiguous()
            x_in = b.t[f"x_in{i}"] = self._cast_in(b, f"feats_c{i}", x_in)
            u = b.get(f"u{i}", (B * Ts[i], d), self.dt)
            ops.gemm(x_in, self.W(f"unify.{i}.weight"), u, bias=self.F(f"unify.{i}.bias"))
            us.append(u)
        kp, mks = None, None
        if masks is not None:
            mks = [self._mask_u8(m) for m in masks]
            kp = b.get("mm_kpm", (B, S), torch.uint8)
        if ex:
            x = ops.enc_frontend_ex_fwd(us, mks, b.get("x0", (B * S, d), self.dt), kp, B, Ts, **self._ex_args(b, B, Ts))
        else:
            temp, labels = self.mm_rows(Ts)
            x = ops.mm_frontend_fwd(us, mks, temp, self.F("modal_emb.modal_emb.weight"), labels, b.get("x0", (B * S, d), self.dt), kp,
                                    B, Ts)
        kpm = (kp, 0) if kp is not None else None     # the [B, S] mask, no shift: both attention paths read it as is
        b.t["kpm_used"] = kpm
        return self._stack_fwd(b, x, B, S, kpm)

    def _ex_args(self, b, B, Ts):
        """What both directions of vct_enc_frontend_ex_* take besides the activations (ops.enc_frontend_ex_fwd / _bwd)."""
        rows, S = self.ex_rows(Ts), sum(t + 1 for t in Ts)
        kw = dict(agg="max" if self.by_max else "avg", labels=rows["labels"],
                  modal_w=self.F("modal_emb.modal_emb.weight") if len(Ts) > 1 else None)
        if self.learned:
            kw.update(tidx=rows["tidx"], emb_w=self.F("temp_emb.embedding.weight"))
        else:
            kw.update(temp=rows["temp"])
        if self.do_norm:
            kw["norm"] = dict(gamma=self.F("norm.weight"), beta=self.F("norm.bias"), mean=b.get("in.mean", (B * S,), torch.float32),
                              rstd=b.get("in.rstd", (B * S,), torch.float32), dropout=self.drop(ENC_IN_SITE))
        return kw

    def _stack_fwd(self, b, x, B, Te, kpm) -> torch.Tensor:
        """The encoder stack on its input x [B*Te, d]: sample-stationary when _ss_ok allows it, else layer by layer."""
        L = self.cfg["layers"]
        if self._ss_ok(Te, 0, B):
            x, mem = self._stack_ss(b, self.lps, self.tags, x, B, Te, self.sites, ln_tag="n2.", ln_name="norm2.",
                                    final="transformer_encoder.norm.", kpm=kpm)
            b.t["x_last"] = x
            return mem
        for l in range(L):
            lp, tag, site = self.lps[l], self.tags[l], self.sites[l]
            b.t[tag + "x"] = x
            x1 = self._attn_ln_fwd(b, tag + "sa.", tag + "n1.", lp + "self_attn.", lp + "norm1.", x, x, B, Te, Te, False, kpm,
                                   site + 1, site + 2)
            f = self._ffn_fwd(b, tag + "ff.", lp, x1, site + 3)
            if l == L - 1:       # norm2 of the last layer + the stack-final norm: one launch
                x, mem = self._ln_ln_fwd(b, tag + "n2.", lp + "norm2.", f, x1, site + 4, "nf.", "transformer_encoder.norm.")
                b.t["x_last"] = x
                return mem
            x = self._ln_fwd(b, tag + "n2.", lp + "norm2.", f, x1, site + 4)
        b.t["x_last"] = x
        return self._ln_fwd(b, "nf.", "transformer_encoder.norm.", x, None, None)

    def _frontend_bwd(self, dx):
        """From the gradient dx [B*S, d] of the stack input: the front end's backward, then the unify weight gradients (and, with
        n >= 2 modalities, the modal-embedding gradient, WRITTEN by vct_mm_frontend_bwd)."""
        b, (B, T), d = self.cur, self.shape, self.cfg["d"]
        if self.mm_Ts is None:
            du = ops.enc_frontend_bwd(dx, b.get("du", (B * T, d), self.dt), B, T)
            self.dw_gemm(du, b.t["x_in"], self.G("unify.0.weight"), bias_grad=self.G("unify.0.bias"))
            return
        Ts = self.mm_Ts
        dus = [b.get(f"du{i}", (B * t, d), self.dt) for i, t in enumerate(Ts)]
        if self.variant:
            # ONE launch (two with the norm: the parameter sums behind the rows); the gradients of temp_emb.embedding.weight and
            # modal_emb are WRITTEN, the norm's partials join the batched LayerNorm-parameter finalize (flush_ln_grads)
            n, S = len(Ts), T + 1
            kw = self._ex_args(b, B, Ts)
            if self.do_norm:
                ws = b.get("in.ln_ws", (B * n * 2 * d,), torch.float32)
                kw.update(dpre=b.get("in.dpre", (B * S, d), torch.float32), param_ws=ws)
                self._ln_pending.append((ws.data_ptr(), self.G("norm.weight").data_ptr(), self.G("norm.bias").data_ptr(), B * n))
            ops.enc_frontend_ex_bwd(dx, dus, B, Ts, us=[b.t[f"u{i}"] for i in range(n)],
                                    d_modal=self.G("modal_emb.modal_emb.weight") if n > 1 else None,
                                    d_emb=self.G("temp_emb.embedding.weight") if self.learned else None, **kw)
        else:
            ops.mm_frontend_bwd(dx, dus, self.G("modal_emb.modal_emb.weight"), self.mm_rows(Ts)[1], B, Ts)
        for i, du in enumerate(dus):
            self.dw_gemm(du, b.t[f"x_in{i}"], self.G(f"unify.{i}.weight"), bias_grad=self.G(f"unify.{i}.bias"))

    def ss_bwd_ok(self) -> bool:
        """The current shape's activation-gradient chain runs as one sample-stationary launch (csrc/vct_layer_ss_bwd.hip)."""
        B, T = self.shape
        return bool(self.fuse_bwd and self._ss_ok(T + 1, 0, B) and self.cfg["layers"] <= 4)

    def backward(self, dmem: torch.Tensor, bucket_ready=None, join: bool = True):
        """join = False (one-launch backward on the main stream, trainer): the weight-gradient GEMMs stay un-joined on the side
        stream; the caller joins before it touches the encoder's gradients."""
        b = self.cur
        B, T = self.shape
        Te, L = T + 1, self.cfg["layers"]
        kpm = b.t["kpm_used"]
        if self.ss_bwd_ok() and dmem.dtype == self.dt:
            # the whole dX chain of the stack in one launch; behind it one grouped weight-gradient launch per layer
            dx = b.get("L0.sa.dx", (B * Te, self.cfg["d"]), self.dt)
            order, after = self._stack_ss_bwd(b, self.lps, self.tags, self.sites, dmem, dx, B, Te, ln_tag="n2.", ln_name="norm2.",
                                              final="transformer_encoder.norm.", kpm=kpm)
            for l, items in zip(order, after):
                for dyv, xv, name in items:
                    self.dw_gemm(dyv, xv, self.G(name + "weight"), bias_grad=self.G(name + "bias"))
                if l > 0:
                    self.flush_dw()
                if bucket_ready is not None and l > 0:
                    self.flush_ln_grads(b)
                    self.bucket_on_side(bucket_ready, "enc_layer", l)
            self._frontend_bwd(dx)
            self.flush_ln_grads(b)
            if join or bucket_ready is not None:
                self.join_side()
            else:
                self.flush_dw()
            if bucket_ready is not None:
                bucket_ready("enc_layer", 0)
            return
        if not self.fuse_ln_ln_bwd:
            dx, _ = self._ln_bwd(b, "nf.", "transformer_encoder.norm.", dmem, b.t["x_last"], None, None)
        for l in reversed(range(L)):
            lp, tag, site = self.lps[l], self.tags[l], self.sites[l]
            x, x1 = b.t[tag + "x"], b.t[tag + "n1.y"]
            if l == L - 1 and self.fuse_ln_ln_bwd:      # stack-final norm + this layer's norm2: one launch
                ds2, df = self._ln_ln_bwd(b, "nf.", "transformer_encoder.norm.", dmem, b.t["x_last"], tag + "n2.", lp + "norm2.",
                                          b.t[tag + "ff.f"], x1, site + 4)
            else:
                ds2, df = self._ln_bwd(b, tag + "n2.", lp + "norm2.", dx, b.t[tag + "ff.f"], x1, site + 4)
            dx1 = self._ffn_bwd(b, tag + "ff.", lp, df, x1, site + 3, ds2)
            ds1, da = self._ln_bwd(b, tag + "n1.", lp + "norm1.", dx1, b.t[tag + "sa.a"], x, site + 2)
            dx = self._attn_block_bwd(b, tag + "sa.", lp + "self_attn.", da, x, x, B, Te, Te, False, kpm, site + 1, True, ds1)
            if l > 0:
                if bucket_ready is None and self.enc_dw_main and self.main_stream is not None:
                    self.flush_dw_across(self.main_stream)      # behind the main stream's tail (vocabulary dW, optimizer pass)
                else:
                    self.flush_dw()       # this layer's weight gradients: one grouped launch beside the next layer
            if bucket_ready is not None and l > 0:
                self.flush_ln_grads(b)
                self.bucket_on_side(bucket_ready, "enc_layer", l)
        self._frontend_bwd(dx)
        self.flush_ln_grads(b)
        if bucket_ready is None and self.enc_dw_main >= 2 and self.main_stream is not None:
            self.flush_dw_across(self.main_stream)       # (A/B: the bottom layer's group too)
        self.join_side()
        if bucket_ready is not None:
            bucket_ready("enc_layer", 0)


class HMMEncoderEngine(EncoderEngine):
    """HMMEncoder: model/MMEncoder.py:313-402 of the reference.  MultiModalEncoder's front end (every option, one stream or several),
    then cfg['layers'] = max(cfg['hmm_layers']) shared layers `trans_enc_layers.{l}.*` with NO stack-final norm.  Stream j goes
    through the last hmm_layers[j] of them: with target[j] = L - hmm_layers[j], layer i reads the previous layer's output on the
    rows of stream j when target[j] < i and the stack input mm_src otherwise -- in the layers before that its rows are still keys
    and values of the other streams, and their outputs are dropped.  The unfused per-layer schedule with ops.hmm_mix_fwd between
    the layers 1 .. max(target); the backward routes each layer's input gradient back (ops.hmm_mix_bwd) and sums the stack
    input's share over the layers max(target) .. 0 in an fp32 accumulator.  Equal depths launch no mix in either direction."""

    def __init__(self, ps, prefix, cfg, seed, pe_buffer: torch.Tensor):
        super().__init__(ps, prefix, cfg, seed, pe_buffer)
        self.lps = [f"trans_enc_layers.{l}." for l in range(cfg["layers"])]
        self._take = {}

    def _ss_ok(self, Lr: int, Lm: int, Bn: int) -> bool:
        """No sample-stationary form of this stack (nor of its backward, nor the one-stream front end folded into that launch)."""
        return False

    @staticmethod
    def take_table(layers, Ts):
        """uint8 [L, S], L = max(layers), S = sum(T_i + 1): take[i, s] = 1 where layer i reads the previous layer's output on row s
        (target[j] = L - layers[j] < i for the stream j that owns s), 0 where it restarts from the stack input."""
        import numpy as np
        if len(layers) != len(Ts):
            raise ValueError(f"hierarchical encoder: {len(layers)} layer counts for {len(Ts)} feature streams")
        L = max(layers)
        target = np.concatenate([np.full(t + 1, L - n, np.int64) for n, t in zip(layers, Ts)])
        return (target[None, :] < np.arange(L)[:, None]).astype(np.uint8)

    def take_rows(self, Ts):
        """(take uint8 [L, S] on the device, max(target)) for the frame counts Ts, built once per frame-count tuple."""
        r = self._take.get(Ts)
        if r is None:
            layers = self.cfg["hmm_layers"]
            r = self._take[Ts] = (torch.from_numpy(self.take_table(layers, Ts)).to(self.dev), max(layers) - min(layers))
        return r

    def _stack_fwd(self, b, x, B, Te, kpm) -> torch.Tensor:
        """The layers on the stack input x [B*Te, d]; returns the memory: the last layer's norm2 output."""
        take, top = self.take_rows(self.mm_Ts if self.mm_Ts is not None else (Te - 1,))
        x0 = x
        for l in range(self.cfg["layers"]):
            lp, tag, site = self.lps[l], self.tags[l], self.sites[l]
            if 1 <= l <= top:
                x = ops.hmm_mix_fwd(x, x0, take[l], b.get(tag + "xin", tuple(x0.shape), self.dt), B, Te)
            b.t[tag + "x"] = x
            x1 = self._attn_ln_fwd(b, tag + "sa.", tag + "n1.", lp + "self_attn.", lp + "norm1.", x, x, B, Te, Te, False, kpm,
                                   site + 1, site + 2)
            f = self._ffn_fwd(b, tag + "ff.", lp, x1, site + 3)
            x = self._ln_fwd(b, tag + "n2.", lp + "norm2.", f, x1, site + 4)
        b.t["x_last"] = x
        return x

    def backward(self, dmem: torch.Tensor, bucket_ready=None, join: bool = True):
        """As EncoderEngine.backward's unfused schedule (side stream, bucket callbacks, join), without a final norm and with the
        row routing's backward behind each layer's dX chain."""
        b = self.cur
        B, T = self.shape
        Te, L = T + 1, self.cfg["layers"]
        kpm = b.t["kpm_used"]
        take, top = self.take_rows(self.mm_Ts if self.mm_Ts is not None else (T,))
        acc = b.get("hmm.acc", (B * Te, self.cfg["d"]), torch.float32) if top > 0 else None
        dx = dmem
        for l in reversed(range(L)):
            lp, tag, site = self.lps[l], self.tags[l], self.sites[l]
            x, x1 = b.t[tag + "x"], b.t[tag + "n1.y"]
            ds2, df = self._ln_bwd(b, tag + "n2.", lp + "norm2.", dx, b.t[tag + "ff.f"], x1, site + 4)
            dx1 = self._ffn_bwd(b, tag + "ff.", lp, df, x1, site + 3, ds2)
            ds1, da = self._ln_bwd(b, tag + "n1.", lp + "norm1.", dx1, b.t[tag + "sa.a"], x, site + 2)
            dx = self._attn_block_bwd(b, tag + "sa.", lp + "self_attn.", da, x, x, B, Te, Te, False, kpm, site + 1, True, ds1)
            if 1 <= l <= top:       # the previous layer's output gets the continuing rows, the accumulator the restarting ones
                dx = ops.hmm_mix_bwd(dx, take[l], acc, B, Te, dy=b.get(tag + "dy", tuple(dx.shape), self.dt), init=(l == top))
            elif l == 0 and top > 0:
                dx = ops.hmm_mix_bwd(dx, None, acc, B, Te, dx0=b.get("hmm.dx0", tuple(dx.shape), self.dt))
            if l > 0:
                if bucket_ready is None and self.enc_dw_main and self.main_stream is not None:
                    self.flush_dw_across(self.main_stream)
                else:
                    self.flush_dw()
            if bucket_ready is not None and l > 0:
                self.flush_ln_grads(b)
                self.bucket_on_side(bucket_ready, "enc_layer", l)
        self._frontend_bwd(dx)
        self.flush_ln_grads(b)
        if bucket_ready is None and self.enc_dw_main >= 2 and self.main_stream is not None:
            self.flush_dw_across(self.main_stream)
        self.join_side()
        if bucket_ready is not None:
            bucket_ready("enc_layer", 0)
