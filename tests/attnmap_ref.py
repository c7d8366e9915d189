"""fp64 numpy reference of vct_attn_weights (include/vct_hip.h) shared by the attention-map tests: the head-averaged attention
probabilities nn.MultiheadAttention returns with need_weights=True, average_attn_weights=True."""
import numpy as np


def attn_weights_ref(q, k, H, causal=False, key_pad=None, shift=0):
    """q [B, Lq, H*hd], k [B, Lk, H*hd] -> W fp64 [B, Lq, Lk] = mean over heads of softmax(q_h k_h^T / sqrt(hd) + mask).
    causal: key j > query i masked.  key_pad: bool [B, Lk - shift], True = padded key (the first `shift` keys are never padded).
    A fully masked row is all zero (the kernels' rule; torch would give NaN)."""
    q, k = np.asarray(q, np.float64), np.asarray(k, np.float64)
    B, Lq, D = q.shape
    Lk, hd = k.shape[1], D // H
    qh = q.reshape(B, Lq, H, hd).transpose(0, 2, 1, 3)
    kh = k.reshape(B, Lk, H, hd).transpose(0, 2, 1, 3)
    s = qh @ kh.transpose(0, 1, 3, 2) / np.sqrt(hd)                  # [B, H, Lq, Lk]
    masked = np.zeros((B, 1, Lq, Lk), bool)
    if causal:
        masked |= (np.arange(Lk)[None, :] > np.arange(Lq)[:, None])[None, None]
    if key_pad is not None:
        kp = np.zeros((B, Lk), bool)
        kp[:, shift:] = np.asarray(key_pad, bool)
        masked |= kp[:, None, None, :]
    s = np.where(masked, -np.inf, s)
    m = s.max(-1, keepdims=True)
    m = np.where(np.isfinite(m), m, 0.0)
    e = np.exp(s - m)
    l = e.sum(-1, keepdims=True)
    p = np.where(l > 0, e / np.where(l > 0, l, 1.0), 0.0)
    return p.mean(1)
