"""What every wrapper family shares: the dropout triple, the row stride of a 2-D view and the stream handle."""
from typing import Optional, Tuple

import torch

from .. import _lib as L

Drop = Optional[Tuple[torch.Tensor, int, float]]  # (seed tensor uint32[1] on device, site id, p)


def _drop(d: Drop):
    if d is None or d[2] <= 0.0:
        return 0, 0, 0.0
    return d[0].data_ptr(), int(d[1]), float(d[2])


def _ld(t: torch.Tensor) -> int:
    assert t.dim() == 2 and t.stride(1) == 1, "row-major 2-D view required"
    return t.stride(0)


def _sptr(stream) -> int:
    return stream.cuda_stream if stream is not None else L.stream_ptr()
