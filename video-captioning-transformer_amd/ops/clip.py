"""Gradient clipping over the flat gradient buffer (csrc/vct_grad_clip.hip): global L2 norm, per-parameter norms, scale / clamp."""
import torch

from .. import _lib as L

GRAD_EPB = 4096      # elements per workgroup (csrc/vct_grad_clip.hip)


def grad_segments_table(segments, device):
    """Device table for grad_sqnorm / grad_clip_apply: segments = [(begin, end)] of flat elements, sorted and disjoint, begin a
    multiple of 4, end > begin and otherwise arbitrary.  Returns (table tensor, entries, workgroups).  ValueError on anything else
    (the kernels trust the table)."""
    segments = [(int(a), int(b)) for a, b in segments]
    if not segments:
        raise ValueError("grad_segments_table: no segments")
    arr = (L.GradSeg * len(segments))()
    blk, prev_end = 0, 0
    for i, (a, b) in enumerate(segments):
        if a < 0 or b <= a:
            raise ValueError(f"segment {i}: [{a}, {b}) is empty or negative")
        if a % 4:
            raise ValueError(f"segment {i}: begin {a} is no multiple of 4 (16-byte vectors)")
        if i and a < segments[i - 1][0]:
            raise ValueError(f"segment {i}: begins at {a}, before segment {i - 1} ({segments[i - 1][0]}): the table must be sorted")
        if a < prev_end:
            raise ValueError(f"segment {i}: [{a}, {b}) overlaps segment {i - 1}, which ends at {prev_end}")
        arr[i].begin, arr[i].end, arr[i].blk0, arr[i].reserved = a, b, blk, 0
        blk += (b - a + GRAD_EPB - 1) // GRAD_EPB
        prev_end = b
    if blk >= 2 ** 31:
        raise ValueError("grad_segments_table: more than 2^31 workgroups")
    table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(device)
    return table, len(segments), blk


def grad_sqnorm_scratch(table, device):
    """The fp64 scratch grad_sqnorm needs for `table`: one partial per workgroup, then one sum per segment."""
    return torch.zeros(table[2] + table[1], dtype=torch.float64, device=device)


def grad_sqnorm(grad, table, partials, seg_norm, clip, state):
    """Two launches: state[0] <- the L2 norm of the segments of the flat fp32 buffer `grad`, state[1] <- the clipping coefficient
    min(1, clip[0] / (norm + 1e-6)), seg_norm[i] <- the norm of segment i.  partials: grad_sqnorm_scratch(table); clip: device fp32 [2]
    = (max_norm, max_value); state: device fp32 [4]."""
    tab, n, blocks = table
    if partials.dtype != torch.float64 or partials.numel() < blocks + n or seg_norm.dtype != torch.float32 or seg_norm.numel() < n \
            or clip.dtype != torch.float32 or clip.numel() < 2 or state.dtype != torch.float32 or state.numel() < 4 \
            or grad.dtype != torch.float32:
        raise ValueError("grad_sqnorm: fp32 grad, fp64 partials [workgroups + segments], fp32 seg_norm [segments], clip [2], state [4]")
    L.check(L.load().vct_grad_sqnorm(grad.data_ptr(), tab.data_ptr(), int(n), int(blocks), partials.data_ptr(), seg_norm.data_ptr(),
                                     clip.data_ptr(), state.data_ptr(), L.stream_ptr()), "vct_grad_sqnorm")


def grad_clip_apply(grad, table, clip, state=None, mode="norm"):
    """One launch, in place: mode 'norm' multiplies every segment element by state[1] (nothing is touched when it is exactly 1),
    mode 'value' clamps to [-clip[1], clip[1]] as torch.clamp does."""
    if mode not in ("norm", "value"):
        raise ValueError(f"grad_clip_apply: mode {mode!r}")
    tab, n, blocks = table
    if grad.dtype != torch.float32 or clip.dtype != torch.float32 or clip.numel() < 2 or (mode == "norm" and (state is None or state.numel() < 4)):
        raise ValueError("grad_clip_apply: fp32 grad, clip [2], and state [4] in norm mode")
    L.check(L.load().vct_grad_clip_apply(grad.data_ptr(), tab.data_ptr(), int(n), int(blocks), 0 if mode == "norm" else 1, clip.data_ptr(),
                                         L.ptr(state), L.stream_ptr()), "vct_grad_clip_apply")
