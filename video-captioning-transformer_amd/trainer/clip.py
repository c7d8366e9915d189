"""Gradient clipping of the training step: by global L2 norm (torch.nn.utils.clip_grad_norm_) or by value (clip_grad_value_), as
two or three launches over the flat gradient buffer between the backward and the optimizer (csrc/vct_grad_clip.hip)."""
import torch

from .. import ops

KEYS = ("max_grad_norm", "clip_grad_value")      # where the settings live: optimizer.param_groups[0]


def check_clip_settings(max_grad_norm=None, clip_grad_value=None):
    """(mode, max_grad_norm, clip_grad_value) with mode None / 'norm' / 'value'.  ValueError: both set, or one that is not a
    number > 0 (NaN included).  max_grad_norm = inf is allowed: the norm is measured and nothing is ever scaled."""
    if max_grad_norm is not None and clip_grad_value is not None:
        raise ValueError("max_grad_norm and clip_grad_value are both set: clip by the global norm OR by value")
    for key, v in zip(KEYS, (max_grad_norm, clip_grad_value)):
        if v is not None and not (isinstance(v, (int, float)) and not isinstance(v, bool) and float(v) > 0.0):      # (NaN > 0 is False)
            raise ValueError(f"{key} must be a number > 0, got {v!r}")
    if max_grad_norm is not None:
        return "norm", float(max_grad_norm), None
    if clip_grad_value is not None:
        return "value", None, float(clip_grad_value)
    return None, None, None


def clip_settings_of(optimizer):
    """check_clip_settings of what optimizer.param_groups[0] holds now (schedulers, load_state_dict and the user write there)."""
    g = optimizer.param_groups[0]
    return check_clip_settings(g.get(KEYS[0]), g.get(KEYS[1]))


class GradClipper:
    """The clipping launches over flat elements [begin, end) of the model's gradient buffer: one segment per parameter, in flat
    order, so that the alignment padding between parameters is never read.  Every device buffer (segment table, the settings block,
    the state, the fp64 partials, the per-parameter norms) is allocated once: recorded launch lists and captured graphs keep valid
    pointers, and follow the settings through the device block."""

    def __init__(self, model, begin: int, end: int):
        ps = model._ps
        self.names, segs = [], []
        for n in ps.names:                                   # (flat order)
            a, k = ps.offsets[n], ps.params[n].numel()
            if k and begin <= a and a + k <= end:
                self.names.append(n)
                segs.append((a, a + k))
        if not segs:
            raise ValueError(f"no parameter inside flat elements [{begin}, {end})")
        dev = ps.gflat.device
        self.grad = ps.gflat
        self.table = ops.grad_segments_table(segs, dev)
        self.partials = ops.grad_sqnorm_scratch(self.table, dev)
        self.seg_norm = torch.zeros(len(segs), dtype=torch.float32, device=dev)
        self.clip = torch.zeros(2, dtype=torch.float32, device=dev)            # {max_norm, max_value}
        self.state = torch.zeros(4, dtype=torch.float32, device=dev)           # {norm, coef, 0, 0}
        self._host = None
        self.mode = None                                     # 'norm' / 'value': what enqueue() issues (set by sync)

    def sync(self, max_norm, max_value):
        """Upload the settings if they changed (host check, rare H2D copy).  Outside any capture, like FusedAdam.sync_hyper."""
        self.mode = "norm" if max_norm is not None else "value"
        h = (float(max_norm or 0.0), float(max_value or 0.0))
        if h != self._host:
            self.clip.copy_(torch.tensor(h, dtype=torch.float32))
            self._host = h

    def enqueue(self):
        """The launches, on the current stream: 'norm' = two for the norm + one that scales; 'value' = one that clamps."""
        if self.mode == "norm":
            ops.grad_sqnorm(self.grad, self.table, self.partials, self.seg_norm, self.clip, self.state)
            ops.grad_clip_apply(self.grad, self.table, self.clip, self.state, "norm")
        else:
            ops.grad_clip_apply(self.grad, self.table, self.clip, None, "value")
