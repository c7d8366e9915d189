"""Element-wise and data-movement helpers: scale, axpby, cache warm-up, casts, row argmax, transpose, seed advance, clip gather."""
from typing import Optional

import torch

from .. import _lib as L
from ._common import _ld


def scale(x: torch.Tensor, s: float):
    """x *= s over a contiguous fp32 range (include/vct_hip.h, vct_scale)."""
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError("scale: a contiguous fp32 tensor")
    L.check(L.load().vct_scale(x.data_ptr(), x.numel(), float(s), L.stream_ptr()), "vct_scale")
    return x


def axpby(out: torch.Tensor, x: torch.Tensor, a: float, y: Optional[torch.Tensor] = None, b: float = 0.0):
    """out = a * x + b * y over contiguous fp32 tensors of one size (y None: a * x; include/vct_hip.h, vct_axpby)."""
    for t in (out, x, y):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != out.numel()):
            raise ValueError("axpby: contiguous fp32 tensors of one size")
    L.check(L.load().vct_axpby(out.data_ptr(), x.data_ptr(), float(a), L.ptr(y), float(b), out.numel(), L.stream_ptr()), "vct_axpby")
    return out


def warm(t: torch.Tensor):
    """Read-only pass over a tensor: pulls it into the memory-side cache for the launch that streams it next (include/vct_hip.h, vct_warm)."""
    L.check(L.load().vct_warm(t.data_ptr(), t.numel() * t.element_size(), L.stream_ptr()), "vct_warm")


def cast(src, dst):
    L.check(L.load().vct_cast(L.dtype_code(src.dtype), L.dtype_code(dst.dtype), src.data_ptr(), dst.data_ptr(),
                              src.numel(), L.stream_ptr()), "vct_cast")
    return dst


def argmax_rows(x, out, cols=None):
    """out: int64 1-D tensor (any stride): out[row] = first index of the row maximum."""
    L.check(L.load().vct_argmax_rows(L.dtype_code(x.dtype), x.shape[0], cols or x.shape[1], x.data_ptr(), _ld(x),
                                     out.data_ptr(), out.stride(0), L.stream_ptr()), "vct_argmax_rows")
    return out


def advance_seed(seed):
    L.check(L.load().vct_advance_seed(seed.data_ptr(), L.stream_ptr()), "vct_advance_seed")


def transpose(src: torch.Tensor, dst: torch.Tensor):
    """dst[c, r] = src[r, c] (bf16; row strides free)."""
    L.check(L.load().vct_transpose(L.dtype_code(src.dtype), src.shape[0], src.shape[1], src.data_ptr(), src.stride(0),
                                   dst.data_ptr(), dst.stride(0), L.stream_ptr()), "vct_transpose")
    return dst


def gather_pad_rows(store: torch.Tensor, offsets: torch.Tensor, idx: torch.Tensor, tmax: int, out_dtype=torch.float32):
    """store fp32 [rows, E] (packed clips), offsets int64 [n+1], idx int64 [B] -> (feat [B, tmax, E], mask bool [B, tmax])."""
    B, E = idx.numel(), store.shape[1]
    out = torch.empty(B, tmax, E, dtype=out_dtype, device=store.device)
    mask = torch.empty(B, tmax, dtype=torch.bool, device=store.device)
    L.check(L.load().vct_gather_pad_rows(L.dtype_code(out_dtype), B, tmax, E, store.data_ptr(), offsets.data_ptr(), idx.data_ptr(),
                                         out.data_ptr(), mask.data_ptr(), L.stream_ptr()), "vct_gather_pad_rows")
    return out, mask
