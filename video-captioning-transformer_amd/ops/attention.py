"""The unfused attention kernels (csrc/vct_attn.hip, csrc/vct_attn_weights.hip): forward, backward and the head-averaged weights."""
import torch

from .. import _lib as L
from ._common import Drop, _drop, _ld


def _attn_desc(dtype, B, H, Lq, Lk, hd, causal, q, k, v, key_pad, dropout):
    d = L.AttnDesc()
    d.dtype, d.B, d.H, d.Lq, d.Lk, d.hd, d.causal = L.dtype_code(dtype), B, H, Lq, Lk, hd, int(causal)
    d.q, d.ldq, d.k, d.ldk, d.v, d.ldv = q.data_ptr(), _ld(q), k.data_ptr(), _ld(k), v.data_ptr(), _ld(v)
    # key_pad: uint8/bool [B, Lk] | (mask [B, Lk - shift], shift) = first `shift` keys never padded | ("ids", ids [B, >=Lk] int64, pad_id)
    if isinstance(key_pad, tuple) and key_pad[0] == "ids":
        _tag, ids, pad_id = key_pad
        assert ids.dtype == torch.int64 and ids.stride(1) == 1 and ids.shape[1] >= Lk
        d.key_ids, d.key_ids_bs, d.pad_id = ids.data_ptr(), ids.stride(0), int(pad_id)
    elif isinstance(key_pad, tuple):
        m, shift = key_pad
        assert m.is_contiguous() and m.element_size() == 1 and tuple(m.shape) == (B, Lk - shift)
        d.key_pad, d.key_pad_shift = m.data_ptr(), int(shift)
    else:
        d.key_pad = L.ptr(key_pad)
    d.seed, d.site, d.p_drop = _drop(dropout)
    return d


def attn_fwd(q, k, v, o, B, H, Lq, Lk, causal=False, key_pad=None, dropout: Drop = None, kv_batch_stride: int = 0):
    """q:[B*Lq, >=H*hd] views (any row stride), k,v:[B*Lk, ..]; o:[B*Lq, H*hd].  key_pad: uint8 [B,Lk].
    kv_batch_stride (elements): K/V live in a cache [B, Lmax, ...] and only the first Lk rows of each batch are read."""
    hd = o.shape[1] // H
    d = _attn_desc(q.dtype, B, H, Lq, Lk, hd, causal, q, k, v, key_pad, dropout)
    d.o, d.ldo = o.data_ptr(), _ld(o)
    d.k_bs = d.v_bs = kv_batch_stride
    L.check(L.load().vct_attn_fwd(d, L.stream_ptr()), "vct_attn_fwd")
    return o


def attn_weights(q, k, w, B, H, Lq, Lk, causal=False, key_pad=None, kv_batch_stride: int = 0):
    """w fp32 [B, Lq, Lk] view (last dimension contiguous, any row / batch stride) = mean over the H heads of
    softmax(q k^T / sqrt(hd) + mask): nn.MultiheadAttention's averaged attention weights (include/vct_hip.h, vct_attn_weights).
    q: [B*Lq, >=H*hd] view, k: [B*Lk, ..] view, key_pad / kv_batch_stride as attn_fwd."""
    assert w.dtype == torch.float32 and tuple(w.shape) == (B, Lq, Lk) and w.stride(2) == 1
    hd = q.shape[1] // H
    src = _attn_desc(q.dtype, B, H, Lq, Lk, hd, causal, q, k, k, key_pad, None)
    d = L.AttnWeightsDesc()
    for f in ("dtype", "B", "H", "Lq", "Lk", "hd", "causal", "key_pad_shift", "q", "ldq", "k", "ldk", "key_pad",
              "key_ids", "key_ids_bs", "pad_id"):
        setattr(d, f, getattr(src, f))
    d.w, d.ldw, d.w_bs = w.data_ptr(), (w.stride(1) if Lq > 1 else Lk), w.stride(0)
    d.k_bs = kv_batch_stride
    L.check(L.load().vct_attn_weights(d, L.stream_ptr()), "vct_attn_weights")
    return w


def attn_bwd(q, k, v, d_o, dq, dk, dv, B, H, Lq, Lk, causal=False, key_pad=None, dropout: Drop = None):
    hd = d_o.shape[1] // H
    d = _attn_desc(q.dtype, B, H, Lq, Lk, hd, causal, q, k, v, key_pad, dropout)
    d.d_o, d.ld_do = d_o.data_ptr(), _ld(d_o)
    d.dq, d.ld_dq, d.dk, d.ld_dk, d.dv, d.ld_dv = dq.data_ptr(), _ld(dq), dk.data_ptr(), _ld(dk), dv.data_ptr(), _ld(dv)
    L.check(L.load().vct_attn_bwd(d, L.stream_ptr()), "vct_attn_bwd")
