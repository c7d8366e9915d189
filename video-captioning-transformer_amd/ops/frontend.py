"""The encoder front ends (single stream, multi-modal, every `mme` option) and the hierarchical encoder's row routing."""
import torch

from .. import _lib as L
from ._common import _drop


def enc_frontend_fwd(u, pe_rows, z, B, T):
    L.check(L.load().vct_enc_frontend_fwd(L.dtype_code(u.dtype), B, T, u.shape[1], u.data_ptr(), pe_rows.data_ptr(),
                                          z.data_ptr(), L.stream_ptr()), "vct_enc_frontend_fwd")
    return z


def enc_frontend_bwd(dz, du, B, T):
    L.check(L.load().vct_enc_frontend_bwd(L.dtype_code(dz.dtype), B, T, dz.shape[1], dz.data_ptr(), du.data_ptr(),
                                          L.stream_ptr()), "vct_enc_frontend_bwd")
    return du


def _mm_desc(dtype, B, d, Ts, labels, n_labels):
    if not 2 <= len(Ts) <= L.MM_MAX_MODAL:
        raise ValueError(f"multi-modal front end: 2..{L.MM_MAX_MODAL} modalities, got {len(Ts)}")
    if labels.dtype != torch.int32 or labels.numel() != sum(t + 1 for t in Ts):
        raise ValueError("multi-modal front end: labels must be int32 [sum(T_i + 1)]")
    desc = L.MmFrontendDesc()
    desc.dtype, desc.n, desc.B, desc.d, desc.n_labels = L.dtype_code(dtype), len(Ts), B, d, n_labels
    for i, t in enumerate(Ts):
        desc.T[i] = int(t)
    desc.labels = labels.data_ptr()
    return desc


def mm_frontend_fwd(us, masks, temp, modal_w, labels, x0, key_pad, B, Ts):
    """Multi-modal front end (include/vct_hip.h, vct_mm_frontend_fwd): us[i] [B*T_i, d] unify outputs, masks[i] uint8 [B, T_i] or
    None, temp fp32 [S, d], modal_w fp32 [n_labels, d], labels int32 [S] -> x0 [B*S, d], key_pad uint8 [B, S] (or None)."""
    d = x0.shape[-1]
    desc = _mm_desc(x0.dtype, B, d, Ts, labels, modal_w.shape[0])
    for i, u in enumerate(us):
        desc.u[i] = u.data_ptr()
        desc.mask[i] = L.ptr(masks[i]) if masks is not None else 0
    desc.temp, desc.modal_w, desc.x0, desc.key_pad = temp.data_ptr(), modal_w.data_ptr(), x0.data_ptr(), L.ptr(key_pad)
    L.check(L.load().vct_mm_frontend_fwd(L.C.byref(desc), L.stream_ptr()), "vct_mm_frontend_fwd")
    return x0


def mm_frontend_bwd(dx, dus, d_modal, labels, B, Ts):
    """Backward of mm_frontend_fwd: dus[i] [B*T_i, d] <- dx [B*S, d]; d_modal fp32 [n_labels, d] is WRITTEN."""
    desc = _mm_desc(dx.dtype, B, dx.shape[-1], Ts, labels, d_modal.shape[0])
    for i, du in enumerate(dus):
        desc.du[i] = du.data_ptr()
    desc.dx, desc.d_modal = dx.data_ptr(), d_modal.data_ptr()
    L.check(L.load().vct_mm_frontend_bwd(L.C.byref(desc), L.stream_ptr()), "vct_mm_frontend_bwd")
    return dus


def _fx_desc(dtype, B, d, Ts, agg, temp, emb_w, tidx, modal_w, labels, norm):
    """The part of vct_enc_frontend_ex_desc both directions share.  agg 'avg' | 'max'; temporal source: temp fp32 [S, d] (fixed table)
    or emb_w fp32 [rows, d] with tidx int32 [S] (learned); modal_w / labels: None with one stream; norm: None or the dict of
    enc_frontend_ex_fwd."""
    n, S = len(Ts), sum(t + 1 for t in Ts)
    if not 1 <= n <= L.MM_MAX_MODAL:
        raise ValueError(f"encoder front end: 1..{L.MM_MAX_MODAL} feature streams, got {n}")
    if (temp is None) == (tidx is None):
        raise ValueError("encoder front end: exactly one temporal source (the fixed table, or the embedding weight with its row indices)")
    if tidx is not None and (tidx.dtype != torch.int32 or tidx.numel() != S):
        raise ValueError("encoder front end: tidx must be int32 [sum(T_i + 1)]")
    if n >= 2 and (labels is None or labels.dtype != torch.int32 or labels.numel() != S):
        raise ValueError("encoder front end: labels must be int32 [sum(T_i + 1)]")
    desc = L.EncFrontendExDesc()
    desc.dtype, desc.n, desc.B, desc.d, desc.agg = L.dtype_code(dtype), n, B, d, L.AGG[agg]
    for i, t in enumerate(Ts):
        desc.T[i] = int(t)
    if tidx is not None:
        desc.temporal, desc.tidx, desc.emb_w, desc.emb_rows = L.TEMPORAL["embedding"], tidx.data_ptr(), L.ptr(emb_w), emb_w.shape[0]
    else:
        desc.temporal, desc.temp = L.TEMPORAL["encoding"], temp.data_ptr()
    if n >= 2:
        desc.labels, desc.modal_w, desc.n_labels = labels.data_ptr(), L.ptr(modal_w), modal_w.shape[0]
    if norm is not None:
        s, site, p = _drop(norm.get("dropout"))
        desc.norm, desc.gamma, desc.beta, desc.mean, desc.rstd = 1, norm["gamma"].data_ptr(), L.ptr(norm.get("beta")), \
            norm["mean"].data_ptr(), norm["rstd"].data_ptr()
        desc.seed, desc.site, desc.p_drop = s, site, p
    return desc


def enc_frontend_ex_fwd(us, masks, x0, key_pad, B, Ts, *, agg="avg", temp=None, emb_w=None, tidx=None, modal_w=None, labels=None,
                        norm=None):
    """Encoder front end with every `mme` option (include/vct_hip.h, vct_enc_frontend_ex_fwd), n >= 1 streams: us[i] [B*T_i, d],
    masks[i] uint8 [B, T_i] or None -> x0 [B*S, d], key_pad uint8 [B, S] (or None).  norm: None, or dict(gamma, beta fp32 [d],
    mean, rstd fp32 [B*S] (written), dropout = (seed, site, p) or None): x0 = dropout(LayerNorm(pre))."""
    desc = _fx_desc(x0.dtype, B, x0.shape[-1], Ts, agg, temp, emb_w, tidx, modal_w, labels, norm)
    for i, u in enumerate(us):
        desc.u[i] = u.data_ptr()
        desc.mask[i] = L.ptr(masks[i]) if masks is not None else 0
    desc.x0, desc.key_pad = x0.data_ptr(), L.ptr(key_pad)
    L.check(L.load().vct_enc_frontend_ex_fwd(L.C.byref(desc), L.stream_ptr()), "vct_enc_frontend_ex_fwd")
    return x0


def enc_frontend_ex_bwd(dx, dus, B, Ts, *, agg="avg", us=None, temp=None, emb_w=None, tidx=None, modal_w=None, labels=None,
                        d_modal=None, d_emb=None, norm=None, dpre=None, param_ws=None):
    """Backward of enc_frontend_ex_fwd: dus[i] [B*T_i, d] <- dx [B*S, d]; d_modal fp32 [n_labels, d] (n >= 2) and d_emb fp32
    [rows, d] (learned temporal) are WRITTEN.  us: the forward's unify outputs (agg 'max' or norm).  norm: the forward's dict
    (gamma, mean, rstd, dropout); then dpre fp32 [B*S, d] and param_ws fp32 [B*n*2*d] receive the pre-norm gradient and the
    norm-parameter partials (ln_param_finalize_batched with B*n rows sums them)."""
    desc = _fx_desc(dx.dtype, B, dx.shape[-1], Ts, agg, temp, emb_w, tidx, modal_w, labels, norm)
    for i, du in enumerate(dus):
        desc.du[i] = du.data_ptr()
        desc.u[i] = us[i].data_ptr() if us is not None else 0
    desc.dx, desc.d_modal, desc.d_emb, desc.dpre, desc.param_ws = dx.data_ptr(), L.ptr(d_modal), L.ptr(d_emb), L.ptr(dpre), L.ptr(param_ws)
    L.check(L.load().vct_enc_frontend_ex_bwd(L.C.byref(desc), L.stream_ptr()), "vct_enc_frontend_ex_bwd")
    return dus


def _hmm_desc(t, B, S, take):
    if t.dim() != 2 or t.shape[0] != B * S:
        raise ValueError(f"hierarchical encoder mix: rows [B*S, d] = [{B * S}, d] expected, got {tuple(t.shape)}")
    if take is not None and (take.dtype != torch.uint8 or take.numel() != S or not take.is_contiguous()):
        raise ValueError("hierarchical encoder mix: take must be contiguous uint8 [S]")
    desc = L.HmmMixDesc()
    desc.dtype, desc.B, desc.S, desc.d, desc.take = L.dtype_code(t.dtype), B, S, t.shape[1], L.ptr(take)
    return desc


def hmm_mix_fwd(y, x0, take, x, B, S):
    """Input of a layer of the hierarchical encoder (include/vct_hip.h, vct_hmm_mix_fwd): x[b, s] = y[b, s] (the previous layer's
    output) where take[s], else x0[b, s] (the stack input); y / x0 / x [B*S, d], take uint8 [S]."""
    desc = _hmm_desc(x, B, S, take)
    desc.y, desc.x0, desc.x = y.data_ptr(), x0.data_ptr(), x.data_ptr()
    L.check(L.load().vct_hmm_mix_fwd(L.C.byref(desc), L.stream_ptr()), "vct_hmm_mix_fwd")
    return x


def hmm_mix_bwd(dx, take, acc, B, S, *, dy=None, dx0=None, init: bool = False):
    """Backward of hmm_mix_fwd from the gradient dx [B*S, d] of a layer's input, acc fp32 [B*S, d]: dy <- dx on the continuing rows
    and 0 on the others, acc <- the restarting rows (init: written, 0 elsewhere; else added to).  At layer 0 (take = None):
    dx0 <- acc + dx, nothing else is written.  Returns dy (or dx0)."""
    if acc.dtype != torch.float32 or tuple(acc.shape) != tuple(dx.shape):
        raise ValueError("hierarchical encoder mix: acc must be fp32 with the shape of dx")
    if (dy is None) == (dx0 is None):
        raise ValueError("hierarchical encoder mix: exactly one of dy (layers above 0) and dx0 (layer 0)")
    desc = _hmm_desc(dx, B, S, take if dx0 is None else None)
    desc.dx, desc.dy, desc.acc, desc.dx0, desc.init = dx.data_ptr(), L.ptr(dy), acc.data_ptr(), L.ptr(dx0), int(bool(init))
    L.check(L.load().vct_hmm_mix_bwd(L.C.byref(desc), L.stream_ptr()), "vct_hmm_mix_bwd")
    return dy if dx0 is None else dx0
