"""Generation controls: the limits, the GenerationControls value object with its device block, and its host restatement."""
import math
import struct

import torch


CONTROLS_NGRAM_MAX = 8
CONTROLS_BANNED_MAX = 32
CONTROLS_THETA_MAX = 16.0
CONTROLS_MAX_LEN = 65          # one history token per lane of a wave: t <= 64


def _f32(x: float) -> float:
    """x rounded to fp32 (round-to-nearest-even), as a Python float."""
    return struct.unpack("<f", struct.pack("<f", float(x)))[0]


class GenerationControls:
    """Four logit rules between the generator and the selection of greedy, beam and sampled decoding; an immutable, validated
    value object.  GenerationControls(min_length=0, no_repeat_ngram_size=0, repetition_penalty=1.0, banned_ids=()).

    Semantics.  At step t (1 <= t <= max_len-1) the decoder chooses column t.  A row's history is h[0 .. t-1]: columns 0 .. t-1
    of its id row, start token included; for a beam slot its ancestors' tokens along the parent back-track, exactly as
    beam_decode_ids back-tracks at the end.  The stage edits the step's logits row in place, in the dtype the step produced (bf16
    or fp32), columns < V only, in this order:
      1. repetition penalty theta = repetition_penalty >= 1 (skipped when theta == 1): for every distinct token v of h, once,
         x = float(logit[v]); x = x * inv_theta if x > 0 else x * theta; rounded to the logits' dtype (round-to-nearest-even).
         theta and inv_theta = fp32(1 / theta) are computed on the host and passed as fp32: two multiplications and no division,
         so the host restatement (apply_controls_host) is exact to the bit.
      2. bans (value -inf): every id of banned_ids; end_id while t <= min_length (a caption has at least min_length tokens
         before its end token); and for n = no_repeat_ngram_size >= 1 and t >= n-1 every h[j], n-1 <= j <= t-1, whose preceding
         n-1 tokens h[j-n+1 .. j-1] equal the last n-1 tokens h[t-n+1 .. t-1] (n = 1 bans every token of the history).
    No element is written twice with different values: a banned token is not penalised first.  A row whose ended / finished flag
    is set is not touched (the selection kernels ignore its logits, and the lookahead steps that run past the stop stay harmless).

    These are the rules of Hugging Face's NoRepeatNGram / MinLength / NoBadWords / RepetitionPenalty logits processors; their
    min_length counts the start token (ours = theirs - 1), and their penalty divides where ours multiplies by inv_theta.

    Limits (ValueError naming the value): 0 <= no_repeat_ngram_size <= 8; 1 <= repetition_penalty <= 16, finite; at most 32
    banned ids, each >= 0; and per call (check): min_length <= max_len - 2, banned ids < V, max_len <= 65 (one history token per
    lane of a wave), V > max_len + len(banned_ids) + 1 (a live row always keeps at least one finite logit)."""
    __slots__ = ("min_length", "no_repeat_ngram_size", "repetition_penalty", "banned_ids")

    def __init__(self, min_length: int = 0, no_repeat_ngram_size: int = 0, repetition_penalty: float = 1.0, banned_ids=()):
        if isinstance(min_length, bool) or int(min_length) != min_length or int(min_length) < 0:
            raise ValueError(f"min_length must be an integer >= 0, got {min_length}")
        n = no_repeat_ngram_size
        if isinstance(n, bool) or int(n) != n or not 0 <= int(n) <= CONTROLS_NGRAM_MAX:
            raise ValueError(f"no_repeat_ngram_size must be an integer in 0..{CONTROLS_NGRAM_MAX}, got {n}")
        try:
            theta = float(repetition_penalty)
        except (TypeError, ValueError):
            raise ValueError(f"repetition_penalty must be a number, got {repetition_penalty!r}") from None
        if not math.isfinite(theta) or not 1.0 <= theta <= CONTROLS_THETA_MAX:
            raise ValueError(f"repetition_penalty must be finite and in 1..{CONTROLS_THETA_MAX:g}, got {repetition_penalty}")
        ids = tuple(banned_ids)
        if len(ids) > CONTROLS_BANNED_MAX:
            raise ValueError(f"banned_ids holds at most {CONTROLS_BANNED_MAX} ids, got {len(ids)}")
        for v in ids:
            if isinstance(v, bool) or int(v) != v or int(v) < 0:
                raise ValueError(f"banned_ids must be integers >= 0, got {v!r}")
        set_ = object.__setattr__
        set_(self, "min_length", int(min_length))
        set_(self, "no_repeat_ngram_size", int(n))
        set_(self, "repetition_penalty", theta)
        set_(self, "banned_ids", tuple(int(v) for v in ids))

    def __setattr__(self, name, value=None):
        raise AttributeError("GenerationControls is immutable")

    __delattr__ = __setattr__

    def _key(self):
        return (self.min_length, self.no_repeat_ngram_size, self.repetition_penalty, self.banned_ids)

    def __eq__(self, other):
        return isinstance(other, GenerationControls) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return (f"GenerationControls(min_length={self.min_length}, no_repeat_ngram_size={self.no_repeat_ngram_size}, "
                f"repetition_penalty={self.repetition_penalty}, banned_ids={self.banned_ids})")

    @property
    def is_noop(self) -> bool:
        """Changes nothing: treated as controls=None everywhere (no extra session, no extra launch)."""
        return self.min_length == 0 and self.no_repeat_ngram_size == 0 and self.repetition_penalty == 1.0 and not self.banned_ids

    @property
    def theta(self) -> float:
        """repetition_penalty as the fp32 the device multiplies by."""
        return _f32(self.repetition_penalty)

    @property
    def inv_theta(self) -> float:
        """fp32(1 / repetition_penalty): what a positive logit is multiplied by."""
        return _f32(1.0 / self.repetition_penalty)

    def check(self, max_len: int, V: int):
        """The limits that depend on the call: ValueError before any device work."""
        if int(max_len) > CONTROLS_MAX_LEN:
            raise ValueError(f"generation controls need max_len <= {CONTROLS_MAX_LEN} (one history token per lane of a wave), got "
                             f"max_len={max_len}")
        if self.min_length > int(max_len) - 2:
            raise ValueError(f"min_length must be in 0..max_len-2 = 0..{int(max_len) - 2}, got min_length={self.min_length}")
        for v in self.banned_ids:
            if v >= V:
                raise ValueError(f"banned_ids must lie in [0, V) = [0, {V}), got {v}")
        if not V > int(max_len) + len(self.banned_ids) + 1:
            raise ValueError(f"generation controls need V > max_len + len(banned_ids) + 1 = {int(max_len) + len(self.banned_ids) + 1} "
                             f"so that a live row always keeps at least one finite logit, got V={V}")
        return self

    def pack(self) -> bytes:
        """The 160-byte device control block of vct_logit_controls (include/vct_hip.h, vct_logit_ctl): {int32 min_length, int32
        ngram, float theta, float inv_theta, int32 n_banned, int32 reserved[3], int32 banned[32]}, little-endian."""
        banned = list(self.banned_ids) + [0] * (CONTROLS_BANNED_MAX - len(self.banned_ids))
        return struct.pack("<iiffi3i32i", self.min_length, self.no_repeat_ngram_size, self.theta, self.inv_theta,
                           len(self.banned_ids), 0, 0, 0, *banned)


def _resolve_controls(controls, max_len: int, V: int):
    """controls=None or a no-op -> None; else the GenerationControls, checked against this call's max_len and V."""
    if controls is None:
        return None
    if not isinstance(controls, GenerationControls):
        raise TypeError(f"controls must be a decode.GenerationControls or None, got {type(controls).__name__}")
    return None if controls.is_noop else controls.check(max_len, V)


def apply_controls_host(logits: torch.Tensor, hist: torch.Tensor, end_id: int, controls: GenerationControls, ended=None, V=None):
    """GenerationControls' rules in torch, on the logits tensor wherever it is: logits [M, >= V] (bf16 or fp32) of step
    t = hist.shape[1], edited IN PLACE in columns < V and returned; hist int64 [M, t] the histories (a beam's already
    back-tracked); ended bool / uint8 [M] (rows that are not touched) or None.  Bit for bit what vct_logit_controls writes."""
    M, t = hist.shape
    V = int(V or logits.shape[1])
    dev = logits.device
    hist = hist.to(dev).long()
    x = logits[:, :V]
    rows = torch.arange(M, device=dev)
    ban = torch.zeros(M, V, dtype=torch.bool, device=dev)
    if controls.banned_ids:
        ban[:, torch.tensor(controls.banned_ids, dtype=torch.long, device=dev)] = True
    if t <= controls.min_length:
        ban[:, int(end_id)] = True
    n = controls.no_repeat_ngram_size
    if n >= 1 and t >= n - 1:
        for j in range(n - 1, t):
            eq = torch.ones(M, dtype=torch.bool, device=dev)
            for i in range(1, n):
                eq &= hist[:, j - i] == hist[:, t - i]
            ban[rows[eq], hist[eq, j]] = True
    new = x
    if controls.repetition_penalty != 1.0:
        seen = torch.zeros(M, V, dtype=torch.bool, device=dev)
        seen[rows[:, None].expand(-1, t), hist] = True
        f = x.float()
        theta = torch.tensor(controls.theta, dtype=torch.float32, device=dev)
        inv_theta = torch.tensor(controls.inv_theta, dtype=torch.float32, device=dev)
        pen = torch.where(f > 0, f * inv_theta, f * theta).to(x.dtype)
        new = torch.where(seen & ~ban, pen, x)
    new = torch.where(ban, torch.full_like(x, float("-inf")), new)
    if ended is not None:
        new = torch.where(ended.to(dev).bool()[:, None], x, new)
    x.copy_(new)
    return logits
