"""MultiModalEncoder -- drop-in for the reference's model/MMEncoder.py:205-276 (`temporal: "encoding"` or `"embedding"`, `aggregation:
"avg"` or `"max"`, do_norm either way; one or more modalities), executed by hand-written gfx950 kernels (engine/encoder.py:
EncoderEngine).  Same constructor signature, same forward signature and return tuple, same state_dict keys for every combination.
HMMEncoder -- the same for the reference's hierarchical encoder (model/MMEncoder.py:313-402; engine/encoder.py: HMMEncoderEngine)."""
from typing import List, Optional

import torch
import torch.nn as nn

from ..engine import EncoderEngine, HMMEncoderEngine, ParamSet, memory_len
from ._params import LayerParams, LinearParams, NormParams, StackParams, sinusoid_table


class TemporalEncoding(nn.Module):
    """Holds the `pe` buffer [1, max_len, d] (model/MMEncoder.py:63-81)."""

    def __init__(self, d_model=512, max_len=512, device=None):
        super().__init__()
        self.register_buffer("pe", sinusoid_table(max_len, d_model, "encoder", device).unsqueeze(0))


class TemporalEmbedding(nn.Module):
    """Holds `embedding.weight` [max_len, d], the learned table of the MMT paper; nn.Embedding's N(0, 1) initialisation and no `pe`
    buffer (model/MMEncoder.py:118-160).  The lookup and its dense gradient run in vct_enc_frontend_ex_*."""

    def __init__(self, d_model=512, max_len=512, device=None):
        super().__init__()
        self.embedding = nn.Embedding(max_len, d_model, device=device)


class ModalEmbedding(nn.Module):
    """Holds `modal_emb.weight`: [2n, d] when modal_different (one row per modality and one per aggregation row), else [n, d];
    nn.Embedding's N(0, 1) initialisation (model/MMEncoder.py:12-24).  The lookup runs in vct_mm_frontend_fwd."""

    def __init__(self, num_modal, d_model=512, modal_different=False, device=None):
        super().__init__()
        self.num_modal, self.embed_size, self.modal_different = num_modal, d_model, modal_different
        self.modal_emb = nn.Embedding(num_modal * 2 if modal_different else num_modal, d_model, device=device)


def grad_ready_order_encoder(prefix, n_layers, n_modal: int = 1, temporal_type: str = "encoding", do_norm: bool = False,
                             layers_at: str = "transformer_encoder.layers.", final_norm: Optional[str] = "transformer_encoder.norm."):
    """layers_at / final_norm: where the state_dict keeps the layers and the stack-final norm (None: the stack has none)."""
    names = [prefix + final_norm + "weight", prefix + final_norm + "bias"] if final_norm else []
    for l in reversed(range(n_layers)):
        lp = f"{prefix}{layers_at}{l}."
        names += [lp + k for k in ("norm2.weight", "norm2.bias", "linear2.weight", "linear2.bias", "linear1.weight",
                                   "linear1.bias", "norm1.weight", "norm1.bias", "self_attn.out_proj.weight",
                                   "self_attn.out_proj.bias", "self_attn.in_proj_weight", "self_attn.in_proj_bias")]
    names += [prefix + "unify.0.weight", prefix + "unify.0.bias"]
    if n_modal > 1:      # after unify.0: the last gradient bucket (MMT4Caption.grad_buckets)
        for i in range(1, n_modal):
            names += [f"{prefix}unify.{i}.weight", f"{prefix}unify.{i}.bias"]
        names.append(prefix + "modal_emb.modal_emb.weight")
    # the front end's own parameters: written by its backward, i.e. with unify.* in the last gradient bucket
    if temporal_type == "embedding":
        names.append(prefix + "temp_emb.embedding.weight")
    if do_norm:
        names += [prefix + "norm.weight", prefix + "norm.bias"]
    return names


def grad_ready_order_hmm_encoder(prefix, n_layers, n_modal: int = 1, temporal_type: str = "encoding", do_norm: bool = False):
    """grad_ready_order_encoder for HMMEncoder's keys: n_layers = max(layer list) layers `trans_enc_layers.{l}.*`, no final norm."""
    return grad_ready_order_encoder(prefix, n_layers, n_modal, temporal_type, do_norm, layers_at="trans_enc_layers.", final_norm=None)


class _EncoderFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mod, feats, mask, *params):
        eng = mod._engine()
        mem = eng.forward(feats, mask, mod.training)
        ctx.mod = mod
        B = feats[0].shape[0] if isinstance(feats, (list, tuple)) else feats.shape[0]
        return mem.view(B, memory_len(feats), -1)

    @staticmethod
    def backward(ctx, dmem):
        mod = ctx.mod
        eng = mod._engine()
        eng.backward(dmem.reshape(-1, dmem.shape[-1]).contiguous())
        mod._ps.install_grads()
        return (None, None, None) + (None,) * len(mod._ps.names)


class MultiModalEncoder(nn.Module):
    layers_at, final_norm = "transformer_encoder.layers.", "transformer_encoder.norm."      # state_dict places (MMT4Caption.grad_buckets)
    _engine_cls, _order = EncoderEngine, staticmethod(grad_ready_order_encoder)

    def __init__(self, d_feats: List[int], d_model: int, nhead: int, dim_feedforward: int = 2048,
                 num_encoder_layers: int = 4, dropout: float = 0.1, activation: str = "gelu", global_type: str = "avg",
                 modal_different: bool = True, temporal_type: str = "embedding", do_norm: bool = False,
                 device=torch.device("cuda"), compute_dtype: torch.dtype = torch.bfloat16):
        super().__init__()
        if len(d_feats) < 1:
            raise ValueError("MultiModalEncoder needs at least one feature stream")
        if global_type not in ("avg", "max"):
            raise NotImplementedError(f"aggregation {global_type!r}: the accelerated path has 'avg' and 'max' (the GRU aggregations "
                                      "are out of scope)")
        if temporal_type not in ("encoding", "embedding"):      # (the reference takes any other string as 'encoding': say so instead)
            raise ValueError(f"temporal {temporal_type!r}: 'encoding' or 'embedding'")
        self.device, self.num_modal, self.do_norm = device, len(d_feats), bool(do_norm)
        depth = self._depth(num_encoder_layers, len(d_feats))
        self.cfg = dict(d=d_model, nhead=nhead, ff=dim_feedforward, layers=depth, dropout=float(dropout),
                        activation=activation, n_modal=len(d_feats), modal_different=bool(modal_different),
                        global_type=global_type, temporal_type=temporal_type, do_norm=bool(do_norm))
        self.compute_dtype = compute_dtype
        self.unify = nn.ModuleList([LinearParams(e, d_model, device) for e in d_feats])
        self.temp_emb = (TemporalEmbedding if temporal_type == "embedding" else TemporalEncoding)(d_model, device=device)
        if self.num_modal > 1:        # (a single modality has no modal embedding, MMEncoder.py:232)
            self.modal_emb = ModalEmbedding(self.num_modal, d_model, modal_different, device)
        self._make_stack(d_model, dim_feedforward, depth, device)
        if self.do_norm:              # LayerNorm (+ Dropout) on the stack input (MMEncoder.py:240-242)
            self.norm = NormParams(d_model, device)
        self._ps: Optional[ParamSet] = None   # set by the owner (MMT4Caption) or lazily for standalone use
        self._prefix = ""
        self._eng: Optional[EncoderEngine] = None
        self._seed = None

    def _depth(self, num_encoder_layers, n_modal) -> int:
        return num_encoder_layers

    def _make_stack(self, d_model, ff, depth, device):
        self.transformer_encoder = StackParams(d_model, ff, depth, False, device)

    def _agg(self, mem, srcs):
        return mem[:, 0]

    # ---- engine plumbing -------------------------------------------------------------------------
    def _bind(self, ps: ParamSet, prefix: str, seed: torch.Tensor, rebuild):
        self._ps, self._prefix, self._seed, self._eng, self._rebuild = ps, prefix, seed, None, rebuild

    def _engine(self) -> EncoderEngine:
        if getattr(self, "_rebuild", None) is not None:
            if not self._ps.intact():
                self._rebuild()
        elif self._ps is None or not self._ps.intact():
            named = dict(self.named_parameters())
            order = self._order("", self.cfg["layers"], self.num_modal, self.cfg["temporal_type"], self.do_norm)
            dev = next(self.parameters()).device
            self._ps = ParamSet([(n, named[n]) for n in order], dev, self.compute_dtype)
            self._prefix, self._eng = "", None
            self._seed = torch.tensor([torch.initial_seed() & 0x7FFFFFFF], dtype=torch.int32, device=dev)
        if self._eng is None:
            self._eng = self._engine_cls(self._ps, self._prefix, self.cfg, self._seed, getattr(self.temp_emb, "pe", None))
        return self._eng

    # ---- reference API ---------------------------------------------------------------------------
    def forward(self, srcs: List[torch.Tensor], src_padding_masks: Optional[List[torch.Tensor]]):
        """srcs: one Tensor[B,T_i,E_i] fp32 per modality; src_padding_masks: one Tensor[B,T_i] bool (True = padded) per modality,
        or None.  Returns (memory[B,S,d], global_masks[B,S] or None, memory[:,0]) like MMEncoder.py:276, S = sum_i (T_i + 1)."""
        if len(srcs) != self.num_modal:
            raise ValueError(f"expected {self.num_modal} feature streams, got {len(srcs)}")
        if self.num_modal == 1:
            feats = srcs[0]
            mask = src_padding_masks[0] if src_padding_masks is not None else None
        else:
            feats = list(srcs)
            mask = list(src_padding_masks) if src_padding_masks is not None else None
        eng = self._engine()
        eng.ps.refresh_shadow()
        mem = _EncoderFn.apply(self, feats, mask, *[self._ps.params[n] for n in self._ps.names])
        mem = mem.float() if mem.dtype != torch.float32 else mem.clone()
        gmask = None
        if src_padding_masks is not None:
            parts = []
            for m in src_padding_masks:
                parts += [torch.zeros(m.shape[0], 1, dtype=torch.bool, device=m.device), m]
            gmask = torch.cat(parts, 1)
        return mem, gmask, self._agg(mem, srcs)


class HMMEncoder(MultiModalEncoder):
    """The reference's hierarchical encoder (model/MMEncoder.py:313-402): MultiModalEncoder's front end and options, then
    max(num_encoder_layers) shared layers `trans_enc_layers.{l}.*` (copies of one layer at construction, like _get_clones) without a
    stack-final norm; stream j passes through the last num_encoder_layers[j] of them (engine/encoder.py: HMMEncoderEngine).
    num_encoder_layers: one positive int per feature stream -- the reference indexes the list by stream (a shorter one is an
    IndexError there, a longer one builds depth nobody uses); anything else is a ValueError here."""
    layers_at, final_norm = "trans_enc_layers.", None
    _engine_cls, _order = HMMEncoderEngine, staticmethod(grad_ready_order_hmm_encoder)

    def __init__(self, d_feats: List[int], d_model: int, nhead: int, dim_feedforward: int, num_encoder_layers: List[int],
                 dropout: float = 0.1, activation: str = "gelu", global_type: str = "avg", modal_different: bool = True,
                 temporal_type: str = "embedding", do_norm: bool = False, device=torch.device("cuda"),
                 compute_dtype: torch.dtype = torch.bfloat16):
        super().__init__(d_feats, d_model, nhead, dim_feedforward, num_encoder_layers, dropout, activation, global_type, modal_different,
                         temporal_type, do_norm, device, compute_dtype)
        self.num_encoder_layers = self.cfg["hmm_layers"] = [int(n) for n in num_encoder_layers]

    def _depth(self, num_encoder_layers, n_modal) -> int:
        ls = num_encoder_layers
        if (not isinstance(ls, (list, tuple)) or len(ls) != n_modal
                or any(isinstance(n, bool) or not isinstance(n, int) or n < 1 for n in ls)):
            raise ValueError(f"HMMEncoder: num_encoder_layers must hold one positive int per feature stream ({n_modal}), got {ls!r}")
        return max(ls)

    def _make_stack(self, d_model, ff, depth, device):
        self.trans_enc_layers = nn.ModuleList([LayerParams(d_model, ff, False, device) for _ in range(depth)])
        for l in range(1, depth):
            self.trans_enc_layers[l].load_state_dict(self.trans_enc_layers[0].state_dict())

    def _agg(self, mem, srcs):
        """torch.sum(torch.cat([rows 0 of each stream], dim=1), dim=1): one scalar per sample, shape [B] (MMEncoder.py:399)."""
        firsts, at = [], 0
        for f in srcs:
            firsts.append(mem[:, at])
            at += f.shape[1] + 1
        return torch.sum(torch.cat(firsts, dim=1), dim=1)
