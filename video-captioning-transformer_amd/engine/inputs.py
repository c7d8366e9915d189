"""Encoder inputs as the engines, the trainer and the decode loops pass them around."""
import torch


# Encoder inputs ("feats" / "mask" below and in decode / trainer / MMT4Caption): one tensor (one modality) or a list with one tensor
# per modality (masks: such a list, or None).
def memory_len(feats) -> int:
    """Encoder memory rows per sample: T + 1 for one modality (a tensor [B, T, E] or a one-element list), sum_i (T_i + 1) for a
    list of modalities (MMEncoder.py:249-265)."""
    if isinstance(feats, (list, tuple)):
        return sum(int(f.shape[1]) + 1 for f in feats)
    return int(feats.shape[1]) + 1


def first_input(feats) -> torch.Tensor:
    """The (first modality's) feature tensor: batch size, device and dtype of an encoder input."""
    return feats[0] if isinstance(feats, (list, tuple)) else feats


def static_inputs(x, contiguous: bool = False):
    """A copy of an encoder input at addresses of its own (None stays None, lists element-wise): what recorded launch lists and
    captured graphs read.  contiguous: dense row-major copies instead of clones that keep the strides."""
    if x is None:
        return None
    if isinstance(x, (list, tuple)):
        return [static_inputs(t, contiguous) for t in x]
    if contiguous:
        out = torch.empty_like(x, memory_format=torch.contiguous_format)
        out.copy_(x)
        return out
    return x.clone()


def stage_inputs(dst, src, non_blocking: bool = False):
    """Copy an encoder input into buffers made by static_inputs, skipping a tensor that already IS its buffer (a producer that
    writes its batches into them)."""
    if isinstance(dst, list):
        for a, b in zip(dst, src):
            stage_inputs(a, b, non_blocking)
    elif dst.data_ptr() != src.data_ptr():
        dst.copy_(src, non_blocking=non_blocking)

