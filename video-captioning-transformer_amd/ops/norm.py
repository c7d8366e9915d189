"""Residual-add + LayerNorm, forward and backward, and the pre-LN norm (csrc/vct_norm.hip, csrc/vct_text.hip)."""
import torch

from .. import _lib as L
from ._common import Drop, _drop


def add_ln_fwd(x, res, gamma, beta, y, mean, rstd, dropout: Drop = None):
    M, dm = x.shape
    s, site, p = _drop(dropout)
    L.check(L.load().vct_add_ln_fwd(L.dtype_code(x.dtype), M, dm, x.data_ptr(), L.ptr(res), gamma.data_ptr(),
                                    beta.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), s, site, p,
                                    L.stream_ptr()), "vct_add_ln_fwd")
    return y


def add_ln_ln_fwd(x, res, gamma, beta, y, mean, rstd, gamma2, beta2, y2, mean2, rstd2, dropout: Drop = None):
    """y = LayerNorm(res + dropout(x)); y2 = LayerNorm2(y) -- a layer's last norm and the stack-final norm in one launch."""
    M, dm = x.shape
    s, site, p = _drop(dropout)
    L.check(L.load().vct_add_ln_ln_fwd(L.dtype_code(x.dtype), M, dm, x.data_ptr(), L.ptr(res), gamma.data_ptr(), beta.data_ptr(),
                                       y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma2.data_ptr(), beta2.data_ptr(),
                                       y2.data_ptr(), mean2.data_ptr(), rstd2.data_ptr(), s, site, p, L.stream_ptr()),
            "vct_add_ln_ln_fwd")
    return y2


def ln_ws_rows(M: int) -> int:
    return int(L.load().vct_ln_ws_rows(M))


def add_ln_bwd(dy, x, res, gamma, mean, rstd, ds, dxo, dgamma, dbeta, param_ws, dropout: Drop = None):
    M, dm = x.shape
    s, site, p = _drop(dropout)
    L.check(L.load().vct_add_ln_bwd(L.dtype_code(x.dtype), M, dm, dy.data_ptr(), x.data_ptr(), L.ptr(res),
                                    gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(), ds.data_ptr(), L.ptr(dxo),
                                    L.ptr(dgamma), L.ptr(dbeta), param_ws.data_ptr(), s, site, p,
                                    L.stream_ptr()), "vct_add_ln_bwd")


def add_ln_ln_bwd(dy2, y, gamma2, mean2, rstd2, param_ws2, x, res, gamma, mean, rstd, ds, dxo, param_ws, dropout: Drop = None):
    """Backward of add_ln_ln_fwd in one launch (include/vct_hip.h, vct_add_ln_ln_bwd): the stack-final norm, then the last layer's norm."""
    M, dm = x.shape
    s, site, p = _drop(dropout)
    L.check(L.load().vct_add_ln_ln_bwd(L.dtype_code(x.dtype), M, dm, dy2.data_ptr(), y.data_ptr(), gamma2.data_ptr(), mean2.data_ptr(),
                                       rstd2.data_ptr(), param_ws2.data_ptr(), x.data_ptr(), L.ptr(res), gamma.data_ptr(), mean.data_ptr(),
                                       rstd.data_ptr(), ds.data_ptr(), L.ptr(dxo), param_ws.data_ptr(), s, site, p, L.stream_ptr()),
            "vct_add_ln_ln_bwd")


def ln_param_finalize_batched(table, n_entries, d):
    """table: int64 device tensor [n_entries, 4] = (param_ws ptr, dgamma ptr, dbeta ptr, ws rows)."""
    L.check(L.load().vct_ln_param_finalize_batched(table.data_ptr(), n_entries, d, L.stream_ptr()), "vct_ln_param_finalize_batched")


def preln_fwd(x, gamma, beta, y):
    """y = LayerNorm(x): x the fp32 residual stream [M, d] of a pre-LN stack, y [M, d] fp32 or bf16 (include/vct_hip.h, vct_preln_fwd)."""
    M, dm = x.shape
    assert x.dtype == torch.float32 and x.is_contiguous() and y.is_contiguous() and tuple(y.shape) == (M, dm)
    assert gamma.dtype == beta.dtype == torch.float32 and gamma.numel() == beta.numel() == dm
    L.check(L.load().vct_preln_fwd(L.dtype_code(y.dtype), M, dm, x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(),
                                   L.stream_ptr()), "vct_preln_fwd")
    return y
