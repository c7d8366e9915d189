"""The caption losses over the vocabulary logits and the per-video sum of sampled rows."""
import torch

from .. import _lib as L
from ._common import _ld


def sce_loss(logits, V, labels, S, pad_id, alpha, loss_out, dlogits, row_ws):
    """logits [N, ld>=V]; labels: int64 2-D view [B, >=S] whose first S columns are the targets."""
    N = logits.shape[0]
    L.check(L.load().vct_sce_loss(L.dtype_code(logits.dtype), N, S, V, logits.data_ptr(), _ld(logits), labels.data_ptr(),
                                  labels.stride(0), int(pad_id), float(alpha), loss_out.data_ptr(), L.ptr(dlogits),
                                  _ld(dlogits) if dlogits is not None else 0, row_ws.data_ptr(), L.stream_ptr()),
            "vct_sce_loss")
    return loss_out


def sce_loss_ls(logits, V, labels, S, pad_id, alpha, smoothing, loss_out, dlogits, row_ws, stats=None):
    """vct_sce_loss with label smoothing on the CE term (include/vct_hip.h, vct_sce_loss_ls).  logits, labels, dlogits as in sce_loss;
    smoothing in [0, 1); row_ws: fp32 [4*N + 2] (4*N + 1 are written); stats: fp32 [2] or None, receives (un-smoothed NLL, token accuracy)."""
    N = logits.shape[0]
    assert row_ws.dtype == torch.float32 and row_ws.is_contiguous() and row_ws.numel() >= 4 * N + 1, (row_ws.shape, N)
    if stats is not None:
        assert stats.dtype == torch.float32 and stats.is_contiguous() and stats.numel() == 2
    L.check(L.load().vct_sce_loss_ls(L.dtype_code(logits.dtype), N, S, V, logits.data_ptr(), _ld(logits), labels.data_ptr(),
                                     labels.stride(0), int(pad_id), float(alpha), float(smoothing), loss_out.data_ptr(), L.ptr(stats),
                                     L.ptr(dlogits), _ld(dlogits) if dlogits is not None else 0, row_ws.data_ptr(), L.stream_ptr()),
            "vct_sce_loss_ls")
    return loss_out


def wce_loss(logits, V, labels, S, pad_id, seq_w, loss_out, dlogits, row_ws, tok_logp=None):
    """Sequence-weighted cross-entropy (include/vct_hip.h, vct_wce_loss).  logits [N, ld>=V]; labels: int64 2-D view [B, >=S] whose
    first S columns are the targets; seq_w: fp32 [N / S] on the device or None (all ones); dlogits: None = forward only;
    tok_logp: fp32 [N] or None."""
    N = logits.shape[0]
    if seq_w is not None:
        assert seq_w.dtype == torch.float32 and seq_w.is_contiguous() and seq_w.numel() * S == N, (seq_w.shape, N, S)
    if tok_logp is not None:
        assert tok_logp.dtype == torch.float32 and tok_logp.is_contiguous() and tok_logp.numel() == N
    L.check(L.load().vct_wce_loss(L.dtype_code(logits.dtype), N, S, V, logits.data_ptr(), _ld(logits), labels.data_ptr(),
                                  labels.stride(0), int(pad_id), L.ptr(seq_w), loss_out.data_ptr(), L.ptr(tok_logp), L.ptr(dlogits),
                                  _ld(dlogits) if dlogits is not None else 0, row_ws.data_ptr(), L.stream_ptr()),
            "vct_wce_loss")
    return loss_out


def group_sum(src, out, B: int, G: int, R: int):
    """out[g*R + r] = sum over n < G of src[(g*G + n)*R + r] (include/vct_hip.h, vct_group_sum): src [B*G*R, d], out [B*R, d],
    contiguous, same dtype."""
    d = src.shape[1]
    assert src.is_contiguous() and out.is_contiguous() and src.dtype == out.dtype
    assert tuple(src.shape) == (B * G * R, d) and tuple(out.shape) == (B * R, d), (src.shape, out.shape, B, G, R)
    L.check(L.load().vct_group_sum(L.dtype_code(src.dtype), B, G, R, d, src.data_ptr(), out.data_ptr(), L.stream_ptr()), "vct_group_sum")
    return out
