"""fp64 torch reference (CPU) of the unfused attention kernels (include/vct_hip.h: vct_attn_fwd, vct_attn_bwd; csrc/vct_attn.hip,
csrc/vct_attn_core.h) for any (B, H, Lq, Lk, hd), shared by tests/test_attention_refusals_cpu.py (which checks THIS file against
float64 autograd and against layer_ss_ref.attn_drop) and tests/test_attention_kernels_gpu.py.  Written from the operation's definition:

    S = q k^T / sqrt(hd), masked (causal: key > query; key padding) -> -inf;   P = softmax(S), a FULLY MASKED ROW IS ALL ZERO
    O = (P o M) V                                    M = the dropout multiplier (0 or the fp32-rounded 1 / (1 - p))
    dV = (P o M)^T dO,   dP = (dO V^T) o M,   D = rowsum(dP o P),   dS = P o (dP - D),   dQ = dS K / sqrt(hd),   dK = dS^T Q / sqrt(hd)

The backward is written out (no autograd) so that the zero-row convention holds in the gradients as well: a fully masked row has
P = 0, hence dS = 0, and contributes nothing to dK and dV.  Operands are [B * L, H * hd] matrices (row b * L + l, head h at columns
h * hd ..), as the kernels take them; everything is computed in float64 from the operands as given (round them first to judge a
bf16 kernel on its own inputs).  The dropout counter hash and the key-padding forms come from layer_ss_ref (drop_mult, key_mask)."""
import math

import numpy as np
import torch

from layer_ss_ref import drop_mult, key_mask  # noqa: F401  (key_mask: re-exported for the tests)

F64 = torch.float64


def _d(x):
    return x.detach().to("cpu").to(F64)


def heads(x, B, L, H):
    """[B * L, H * hd] -> [B, H, L, hd] (float64, CPU)."""
    x = _d(x)
    return x.reshape(B, L, H, x.shape[1] // H).transpose(1, 2)


def flat(t):
    """[B, H, L, hd] -> [B * L, H * hd]."""
    B, H, L, hd = t.shape
    return t.transpose(1, 2).reshape(B * L, H * hd)


def masked(B, Lq, Lk, causal=False, kpm=None):
    """bool [B, 1, Lq, Lk], True = the key takes no part: causal (key > query, also when Lq != Lk) or padded (kpm bool [B, Lk])."""
    m = torch.zeros(B, 1, Lq, Lk, dtype=torch.bool)
    if causal:
        m = m | torch.triu(torch.ones(Lq, Lk, dtype=torch.bool), 1)
    if kpm is not None:
        m = m | kpm.cpu().bool()[:, None, None, :]
    return m


def scores(q, k, B, H, Lq, Lk):
    """Scaled scores [B, H, Lq, Lk], unmasked."""
    qh, kh = heads(q, B, Lq, H), heads(k, B, Lk, H)
    return qh @ kh.transpose(-1, -2) / math.sqrt(qh.shape[-1])


def probs(q, k, B, H, Lq, Lk, causal=False, kpm=None):
    """softmax(q k^T / sqrt(hd)) under the causal mask and the key padding -> [B, H, Lq, Lk]; a fully masked row is all zero."""
    s = scores(q, k, B, H, Lq, Lk).masked_fill(masked(B, Lq, Lk, causal, kpm), float("-inf"))
    m = s.amax(-1, keepdim=True)
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    return torch.where(l > 0, e / torch.where(l > 0, l, torch.ones_like(l)), torch.zeros_like(e))


def mult(seed, site, p, B, H, Lq, Lk):
    """Dropout multiplier of the probabilities [B, H, Lq, Lk]: counter ((b * H + h) * Lq + query) * Lk + key, wrapped at 2^32;
    all ones without a seed or with p <= 0."""
    idx = (np.arange(B * H * Lq * Lk, dtype=np.uint64) & np.uint64(0xFFFFFFFF)).reshape(B, H, Lq, Lk)
    return torch.from_numpy(drop_mult(seed, site, p, idx)).to(F64)


def forward(q, k, v, B, H, Lq, Lk, causal=False, kpm=None, M=None):
    """O = (P o M) V -> [B * Lq, H * hd]."""
    p = probs(q, k, B, H, Lq, Lk, causal, kpm)
    if M is not None:
        p = p * M
    return flat(p @ heads(v, B, Lk, H))


def backward(q, k, v, do, B, H, Lq, Lk, causal=False, kpm=None, M=None):
    """(dQ [B * Lq, H * hd], dK [B * Lk, H * hd], dV [B * Lk, H * hd]) of sum(O o dO), by the explicit formulas of the module docstring."""
    p = probs(q, k, B, H, Lq, Lk, causal, kpm)
    M = torch.ones_like(p) if M is None else M
    qh, kh, vh, doh = heads(q, B, Lq, H), heads(k, B, Lk, H), heads(v, B, Lk, H), heads(do, B, Lq, H)
    scale = 1.0 / math.sqrt(qh.shape[-1])
    dv = (p * M).transpose(-1, -2) @ doh
    dp = (doh @ vh.transpose(-1, -2)) * M
    ds = p * (dp - (dp * p).sum(-1, keepdim=True))
    return flat(scale * (ds @ kh)), flat(scale * (ds.transpose(-1, -2) @ qh)), flat(dv)
