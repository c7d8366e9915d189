"""Greedy decoding (reference: model/MMT4Caption.py:146-184, model/CapDecoder.py:62-79).

Two implementations with identical results (tests/test_model_gpu.py):
  * `greedy_decode_ids_reference_algorithm`: the reference's O(L^2) loop -- every step re-runs the whole
    decoder over all tokens so far -- on the HIP kernels; one host sync per token like the reference's
    `.tolist()` (MMT4Caption.py:168).
  * `greedy_decode_ids` (default): KV cache (self-attention K/V per layer [B, Lmax, 2d], cross-attention
    K/V of the memory computed once), ONE new token per step, the per-token kernel sequence captured
    in a hipGraph per position and replayed; end-of-sequence bookkeeping stays on the device and the
    host reads it `lookahead` steps behind the launch front, so the device never idles on the check.
    The reference's stop rule (stop when EVERY row has emitted [SEP] at least once) is honoured by
    truncating the id matrix at that step.

Beam search (`beam_decode_ids`, `beam_decode_ids_reference_algorithm`): the reference has none (MMT4Caption.py:186 is a stub,
predict_video.py:170's `--beam` says "not support yet"); the semantics are stated in `beam_decode_ids`.

Sampling (`sample_decode_ids`, `sample_decode_ids_reference_algorithm`): temperature, top-k and nucleus draws, N captions
per video with their log-probabilities; the reference has none either, the semantics are stated in `sample_decode_ids`.

Generation controls (`GenerationControls`, `apply_controls_host`): minimum length, no-repeat n-gram ban, repetition penalty and
banned ids, applied to the step's logits on the device in front of the selection of all three decoders (`controls=`); the
reference has none, the semantics are stated in `GenerationControls`."""
import math
import struct

import torch

from . import ops
from .engine import SAMPLE_SITE, BeamDecodeState, DecodeState, SampleDecodeState, first_input as _first, memory_len, stage_inputs, static_inputs
from .utils import capture_graph


def _inputs_key(feats, mask):
    if isinstance(feats, (list, tuple)):
        return (tuple((tuple(f.shape), f.dtype) for f in feats), mask is not None)
    return (tuple(feats.shape), feats.dtype, mask is not None)


# ---- generation controls -------------------------------------------------------------------------------------------------------
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


@torch.no_grad()
def greedy_decode_ids_reference_algorithm(model, feats: torch.Tensor, mask, max_len: int = 30, controls=None) -> torch.Tensor:
    """controls: GenerationControls applied to every step's logits by apply_controls_host."""
    pre = model.cap_preprocessor
    model._ps.refresh_shadow()
    model._ps.refresh_lazy_transposed()
    enc, dec = model.video_encoder._engine(), model.cap_decoder._engine()
    B, Te, dev = _first(feats).shape[0], memory_len(feats), _first(feats).device
    controls = _resolve_controls(controls, max_len, dec.V)
    mem = enc.forward(feats, mask, False)
    ys = torch.full((B, max_len), pre.pad_id, dtype=torch.long, device=dev)
    ys[:, 0] = pre.start_id
    ended = torch.zeros(B, dtype=torch.bool, device=dev)
    t = 1
    for _ in range(max_len - 1):
        logits = dec.decode_word(mem, B, Te, ys[:, :t])
        if controls is not None:
            apply_controls_host(logits, ys[:, :t], pre.end_id, controls, ended, V=dec.V)
        ops.argmax_rows(logits, ys[:, t], cols=dec.V)
        ended |= ys[:, t] == pre.end_id
        t += 1
        if bool(ended.all()):
            break
    return ys[:, :t].clone()


def _session(model, dec, B, Te, max_len, return_attn: bool = False, controls: bool = False) -> DecodeState:
    cache = model.__dict__.setdefault("_decode_sessions", {})
    # (graphs bake pointers and launches: a session that returns attention maps is another session, and one without never
    # captures the extra launches)
    # (the same for generation controls: their session captures the vct_logit_controls launch, one without is what it always was)
    key = (B, Te, max_len, dec.dt) + (("attn",) if return_attn else ()) + (("ctl",) if controls else ())
    st = cache.get(key)
    if st is None:
        if len(cache) > 3:
            cache.clear()
        st = cache[key] = DecodeState(dec, B, Te, max_len, return_attn=return_attn, controls=controls)
    return st


def _no_beam_attn(return_attn: bool):
    if return_attn:
        raise ValueError("return_attn is not supported by beam search: the maps would have to follow the beams' parent "
                         "back-track; use greedy_decode_ids(return_attn=True)")


@torch.no_grad()
def greedy_decode_ids(model, feats: torch.Tensor, mask, max_len: int = 30, use_graphs: bool = True,
                      sync_every: int = 4, lookahead: int = 3, return_attn: bool = False, controls=None):
    """Returns ys int64 [B, <= max_len], identical to the reference loop's id matrix.  return_attn: (ys, maps) with maps fp32
    [B, layers, ys.shape[1] - 1, Te]: row t-1 of layer l = the head-averaged cross-attention of the token consumed at step t
    (what predict_video.py --vis_attn records, predict_video.py:43-79); rows of a caption that has already ended hold what the
    step computed, as in the reference.

    The host never waits for the step it has just launched: it keeps `lookahead` token steps queued and, every `sync_every`
    steps, reads the device-side "every caption has ended at step s" word as of the step that left the queue (a copy on a second
    stream issued once the host has seen THAT step's event complete) -- the reference syncs on every token (`.tolist()`, MMT4Caption.py:168).  A
    caption batch that ends at step s therefore costs at most s + lookahead steps; the id matrix is truncated at s.

    controls: a GenerationControls (None or a no-op: nothing changes, not one launch).  Every step's arg-max is then taken from
    the processed logits.  A session with controls is its own session (one more launch per step, vct_logit_controls, in its
    graphs); the settings live in a device block, so that session serves every setting without recapture.  Batch 1 leaves the
    block step for the gemv step, as every selection stage other than the fused greedy one does."""
    dec = model.cap_decoder._engine()
    controls = _resolve_controls(controls, max_len, dec.V)
    st = _session(model, dec, _first(feats).shape[0], memory_len(feats), max_len, return_attn, controls is not None)
    if controls is not None:
        st.set_controls(controls)
    stop = _run_session(model, st, feats, mask, max_len, use_graphs, sync_every, lookahead, dec.decode_begin, dec.decode_step)
    if return_attn:
        return st.ys[:, :stop + 1].clone(), st.attn_maps[:, :, :stop].clone()
    return st.ys[:, :stop + 1].clone()


def _run_session(model, st, feats, mask, max_len, use_graphs, sync_every, lookahead, begin, step) -> int:
    """The token loop shared by greedy and beam decoding: prologue (encoder + begin), one captured graph per position, the
    device-side stop word polled `lookahead` steps behind the launch front.  Returns the last step to keep."""
    pre = model.cap_preprocessor
    model._ps.refresh_shadow()
    model._ps.refresh_lazy_transposed()
    enc = model.video_encoder._engine()
    stamp = model._ps.stamp
    if st.__dict__.get("weights_stamp") != stamp:      # graphs bake weight pointers only, but keep it simple and safe
        st.weights_stamp = stamp
    on_gpu = _first(feats).device.type == "cuda"
    if on_gpu and st.__dict__.get("poll_stream") is None:
        st.poll_stream = torch.cuda.Stream(device=_first(feats).device)
        st.poll_host = torch.empty(1, dtype=torch.long).pin_memory()
        st.events = [torch.cuda.Event() for _ in range(max_len)]
    if use_graphs and on_gpu:
        # the prologue (encoder forward over the batch, cross-attention K/V of the memory for every layer, cache / flag reset:
        # ~40 launches, host-bound at 0.33 ms when issued one by one) is ONE captured graph too; the inputs go through static
        # copies.  It bakes pointers into the engines' shared grow-only buffers: re-captured whenever any of them grew.
        key = _inputs_key(feats, mask)
        bg = st.__dict__.get("begin")
        if bg is None or bg["key"] != key or bg["gen"] != model._ps.ctx.generation:
            fin, min_ = static_inputs(feats, True), static_inputs(mask, True)
            begin(st, enc.forward(fin, min_, False), pre.start_id, pre.pad_id)      # warm-up: allocates
            g = torch.cuda.CUDAGraph()
            with capture_graph(g):
                begin(st, enc.forward(fin, min_, False), pre.start_id, pre.pad_id)
            st.begin = {"key": key, "gen": model._ps.ctx.generation, "g": g, "fin": fin, "min": min_}
        else:
            stage_inputs(bg["fin"], feats)
            if mask is not None:
                stage_inputs(bg["min"], mask)
            bg["g"].replay()
    else:
        begin(st, enc.forward(feats, mask, False), pre.start_id, pre.pad_id)
    stop = max_len

    def ended_as_of(step: int) -> int:
        """all_ended_at once `step` has run (later steps may still be in flight: the word only ever decreases to the FIRST step
        at which every row had ended, so a value read early is either max_len or final)."""
        st.events[step].synchronize()       # the HOST waits for that step (later steps stay queued on the device) ...
        with torch.cuda.stream(st.poll_stream):
            # ... so the copy needs no device-side dependency: a cross-stream wait on an event that is still pending costs
            # ~0.8 ms of latency on this runtime (tools/decode_loop_probe2.py), an independent 8-byte copy 20 us
            st.poll_host.copy_(st.all_ended_at, non_blocking=True)
        st.poll_stream.synchronize()
        return int(st.poll_host[0])

    for t in range(1, max_len):
        if use_graphs:
            g = st.graphs.get(t)
            if g is None:
                step(st, t, pre.end_id)         # warm-up run (allocates the step's temporaries)
                # the warm-up already wrote ys[:, t]; capture replays the same work
                g = torch.cuda.CUDAGraph()
                with capture_graph(g):
                    step(st, t, pre.end_id)
                st.graphs[t] = g
            else:
                g.replay()
        else:
            step(st, t, pre.end_id)
        if not on_gpu:
            continue
        if t % sync_every == 0 or t == max_len - 1:
            st.events[t].record()                          # only the steps that will be polled: an event between two graph
        done = t - lookahead                               # launches costs the device ~15 us

        if done >= 1 and (done % sync_every == 0):
            s = ended_as_of(done)
            if s < max_len:
                stop = s
                break
    else:
        if on_gpu:
            stop = min(stop, ended_as_of(max_len - 1))
    return min(stop, max_len - 1)


@torch.no_grad()
def teacher_forced_next_ids(model, feats: torch.Tensor, mask, prefix_ids: torch.Tensor, steps: int, return_logits: bool = False,
                            return_attn: bool = False):
    """The KV-cache token step of greedy_decode_ids (same kernels, same cache) with the CONSUMED token of every step forced to
    `prefix_ids[:, t - 1]` instead of the step's own previous prediction: returns the predicted next ids [B, steps]
    (column t - 1 = arg-max after consuming prefix_ids[:, :t]).  This is CapDecoder.decode_word + torch.max of the reference
    (CapDecoder.py:62-79, MMT4Caption.py:164-165) evaluated along a given caption -- what a low-precision path can be held
    to where free-running ids would diverge after the first unresolvable logit gap.  return_logits: also the fp32 logits
    [B, steps, V] of every step.  return_attn: also (last) the cross-attention maps fp32 [B, layers, steps, Te] of greedy_decode_ids."""
    pre = model.cap_preprocessor
    model._ps.refresh_shadow()
    model._ps.refresh_lazy_transposed()
    enc, dec = model.video_encoder._engine(), model.cap_decoder._engine()
    B, dev = _first(feats).shape[0], _first(feats).device
    st = DecodeState(dec, B, memory_len(feats), steps + 1, return_attn=return_attn)
    dec.decode_begin(st, enc.forward(feats, mask, False), pre.start_id, pre.pad_id)
    out = torch.empty(B, steps, dtype=torch.long, device=dev)
    logits = torch.empty(B, steps, dec.V, dtype=torch.float32, device=dev) if return_logits else None
    for t in range(1, steps + 1):
        st.ys[:, t - 1] = prefix_ids[:, t - 1]
        dec.decode_step(st, t, pre.end_id)
        out[:, t - 1] = st.ys[:, t]
        if return_logits:
            logits[:, t - 1] = st.last_logits[:, :dec.V].float()
    res = (out, logits) if return_logits else (out,)
    if return_attn:
        res = res + (st.attn_maps[:, :, :steps].clone(),)
    return res if len(res) > 1 else res[0]


def _beam_session(model, dec, B, K, Te, max_len, controls: bool = False) -> BeamDecodeState:
    cache = model.__dict__.setdefault("_decode_sessions", {})
    key = ("beam", B, K, Te, max_len, dec.dt) + (("ctl",) if controls else ())         # never a greedy session's key
    st = cache.get(key)
    if st is None:
        if len(cache) > 3:
            cache.clear()
        st = cache[key] = BeamDecodeState(dec, B, K, Te, max_len, controls=controls)
    return st


def _beam_finish(ids: torch.Tensor, scores: torch.Tensor, B: int, K: int, end_id: int, length_penalty: float, return_all: bool):
    """ids [B*K, L'] (slot order), raw scores fp32 [B*K] -> the slots of each video sorted by s / n^alpha (descending, ties to
    the lower slot), n = generated tokens up to and including the first end_id (all of them if none)."""
    gen = ids[:, 1:] == end_id
    n_all = ids.shape[1] - 1
    first = torch.where(gen.any(1), gen.int().argmax(1) + 1, torch.full_like(gen[:, 0], n_all, dtype=torch.long))
    final = scores.float() / first.float().pow(float(length_penalty))
    final = final.view(B, K)
    final, order = torch.sort(final, dim=1, descending=True, stable=True)
    ids = ids.view(B, K, -1).gather(1, order[:, :, None].expand(-1, -1, ids.shape[1]))
    if return_all:
        return ids, final
    return ids[:, 0].contiguous()


@torch.no_grad()
def beam_decode_ids(model, feats: torch.Tensor, mask, beam_size: int, max_len: int = 30, length_penalty: float = 1.0,
                    use_graphs: bool = True, return_all: bool = False, sync_every: int = 4, lookahead: int = 3,
                    return_attn: bool = False, controls=None):
    """Beam search on the KV-cached decode step.  Returns the best ids int64 [B, L'] (L' <= max_len), or with return_all
    (ids [B, K, L'], final scores fp32 [B, K]), each video's beams sorted best first.

    Semantics (fixed-width beams, finished hypotheses frozen -- NOT a separate finished pool as in Hugging Face's generate):
    K = beam_size (1 <= K <= 16, K <= V) slots per video, each a token history, a cumulative fp32 score s and a finished flag.
    Start: every slot is [start_id], unfinished, s = 0 for slot 0 and -inf for the others.  Step t = 1 .. max_len-1:
    logp[k, v] = logit[k, v] - logsumexp(logit[k, :V]) in fp32 (logits as the decode step produces them: bf16 on the bf16
    paths); an unfinished slot offers the V candidates (k, v) valued s[k] + logp[k, v], a finished slot the one candidate
    (k, pad_id) valued s[k]; the K highest values (ties: smaller flat index k*V + v) become the new slots in rank order,
    each its parent's history + v, score = the value, finished = parent finished or v == end_id.  Stop at the first step
    after which every slot of every video is finished, or at max_len-1 (greedy's stop rule on beams; the id matrix is cut
    there).  Final score s / n^length_penalty, n = generated tokens up to and including the first end_id (all of them for a
    slot that never finished); slots sorted by it, descending, ties to the lower slot.  Layout as greedy's:
    [start, tokens, end, pad...] (a finished beam appends pad_id where greedy appends arg-max tokens).

    K = 1 gives greedy_decode_ids' ids up to and including each row's first end_id, and the same length -- except where an fp32
    rounding coincidence turns two distinct logits into equal logp (the kernel ranks a row's candidates by logit).

    One captured hipGraph per position (it bakes the ping-pong side of the cache), the begin graph and the stop polling of
    greedy_decode_ids.  The batch-1 block step is greedy-only: beams run on the gemv (B*K = 1), fused (bf16, 2..256 rows) or
    generic batched step.  return_attn=True raises ValueError (attention maps are a greedy-decode feature).

    controls: a GenerationControls (None or a no-op: nothing changes).  Each slot's logits are processed with the slot's own
    back-tracked history before logp is formed, so the beam scores are sums of log-probabilities under the CONTROLLED
    distribution (a banned continuation scores -inf and is never selected while a finite one exists).  A session with controls
    is its own session, as in greedy_decode_ids."""
    _no_beam_attn(return_attn)
    pre = model.cap_preprocessor
    dec = model.cap_decoder._engine()
    K = int(beam_size)
    if not 1 <= K <= 16 or K > dec.V:
        raise ValueError(f"beam_size must be in 1..16 and <= the vocabulary size, got {beam_size}")
    controls = _resolve_controls(controls, max_len, dec.V)
    B, dev = _first(feats).shape[0], _first(feats).device
    st = _beam_session(model, dec, B, K, memory_len(feats), max_len, controls is not None)
    if controls is not None:
        st.set_controls(controls)
    stop = _run_session(model, st, feats, mask, max_len, use_graphs, sync_every, lookahead, dec.beam_begin, dec.beam_step)
    # back-track the parent rows once: column t of slot j is the token appended at step t by the slot's ancestor
    M = B * K
    ids = torch.empty(M, stop + 1, dtype=torch.long, device=dev)
    ids[:, 0] = pre.start_id
    r = torch.arange(M, device=dev)
    for t in range(stop, 0, -1):
        ids[:, t] = st.ys[r, t]
        r = st.parents[t].long()[r]
    # steps that ran past `stop` (lookahead) saw only finished slots, already in rank order: they left the scores as they were
    return _beam_finish(ids, st.scores.clone(), B, K, pre.end_id, length_penalty, return_all)


def _select_ref(vals: torch.Tensor, valid: torch.Tensor, K: int):
    """Host-side selection of one step for every video: vals / valid [B, K*V] -> (flat indices [B, K], values [B, K], margin
    between the K-th and (K+1)-th candidate, inf where there is no (K+1)-th).  Stable sorts: value descending, flat index
    ascending on ties, invalid entries last."""
    v = torch.where(valid, vals, torch.full_like(vals, float("-inf")))
    order = torch.sort(v, dim=1, descending=True, stable=True)[1]
    order = order.gather(1, torch.sort(valid.gather(1, order).int(), dim=1, descending=True, stable=True)[1])
    top = order[:, :K + 1]
    tv = v.gather(1, top)
    ok = valid.gather(1, top)
    margin = float("inf")
    if top.shape[1] > K:
        gap = (tv[:, K - 1].double() - tv[:, K].double())[ok[:, K] & torch.isfinite(tv[:, K])]
        if gap.numel():
            margin = float(gap.min())
    return top[:, :K], tv[:, :K], margin


@torch.no_grad()
def beam_decode_ids_reference_algorithm(model, feats: torch.Tensor, mask, beam_size: int, max_len: int = 30,
                                        length_penalty: float = 1.0, return_all: bool = False, return_attn: bool = False,
                                        controls=None):
    """beam_decode_ids without the KV cache: every step re-runs the whole decoder (dec.decode_word) on the reordered [B*K, t]
    histories and selects on the host in torch by the same rule.  Returns (result as beam_decode_ids, min margin): the smallest
    gap between the K-th and (K+1)-th candidate value over every video and step (where a test may not expect ids to agree).
    controls: GenerationControls applied to every step's logits (in the dtype the decoder produced) by apply_controls_host."""
    _no_beam_attn(return_attn)
    pre = model.cap_preprocessor
    model._ps.refresh_shadow()
    model._ps.refresh_lazy_transposed()
    enc, dec = model.video_encoder._engine(), model.cap_decoder._engine()
    K, V = int(beam_size), dec.V
    if not 1 <= K <= 16 or K > V:
        raise ValueError(f"beam_size must be in 1..16 and <= the vocabulary size, got {beam_size}")
    controls = _resolve_controls(controls, max_len, V)
    B = _first(feats).shape[0]
    M, Te, dev = B * K, memory_len(feats), _first(feats).device
    mem = enc.forward(feats, mask, False)
    d = mem.shape[-1]
    mem_rep = mem.reshape(B, 1, Te, d).expand(-1, K, -1, -1).reshape(M * Te, d).contiguous()
    hist = torch.full((M, 1), pre.start_id, dtype=torch.long, device=dev)
    s = torch.full((B, K), float("-inf"), dtype=torch.float32, device=dev)
    s[:, 0] = 0.0
    s = s.reshape(M)
    fin = torch.zeros(M, dtype=torch.bool, device=dev)
    rows = torch.arange(B, device=dev)[:, None] * K
    min_margin = float("inf")
    for _ in range(max_len - 1):
        logits = dec.decode_word(mem_rep, M, Te, hist)
        if controls is not None:
            apply_controls_host(logits, hist, pre.end_id, controls, fin, V=V)
        logits = logits.float()
        logp = logits - torch.logsumexp(logits, dim=1, keepdim=True)
        vals = s[:, None] + logp
        valid = (~fin)[:, None].expand(-1, V).clone()
        frozen = torch.full_like(vals, float("-inf"))
        frozen[:, pre.pad_id] = s
        vals = torch.where(fin[:, None], frozen, vals)
        valid[fin, pre.pad_id] = True
        flat, val, margin = _select_ref(vals.view(B, K * V), valid.view(B, K * V), K)
        min_margin = min(min_margin, margin)
        parent = (rows + flat // V).reshape(M)
        tok = (flat % V).reshape(M)
        hist = torch.cat([hist[parent], tok[:, None]], 1)
        s = val.reshape(M)
        fin = fin[parent] | (tok == pre.end_id)
        if bool(fin.all()):
            break
    return _beam_finish(hist, s, B, K, pre.end_id, length_penalty, return_all), min_margin


# ---- sampling ------------------------------------------------------------------------------------------------------------------
SAMPLE_TOP_K_MAX = 64


def _check_sample_args(num_samples, temperature, top_k, top_p):
    """The range checks of sampled decoding: ValueError before any device work."""
    if int(num_samples) != num_samples or int(num_samples) < 1:
        raise ValueError(f"num_samples must be an integer >= 1, got {num_samples}")
    t = float(temperature)
    if not math.isfinite(t) or t <= 0.0:
        raise ValueError(f"temperature must be finite and > 0, got {temperature}")
    if int(top_k) != top_k or not 0 <= int(top_k) <= SAMPLE_TOP_K_MAX:
        raise ValueError(f"top_k must be in 0..{SAMPLE_TOP_K_MAX} (0 = the whole vocabulary), got {top_k}")
    p = float(top_p)
    if not (0.0 < p <= 1.0):
        raise ValueError(f"top_p must be in (0, 1], got {top_p}")
    if p < 1.0 and int(top_k) == 0:
        raise ValueError("top_p < 1 needs top_k >= 1: the nucleus is taken within the top-k candidates (a nucleus over the whole "
                         "vocabulary is not implemented and is not approximated silently); pass top_k (at most 64)")


def _draw_seed(seed) -> int:
    """seed=None: one draw from torch's default generator (torch.manual_seed makes a run reproducible); else as given."""
    if seed is None:
        return int(torch.randint(0, 2 ** 31 - 1, (1,)).item())
    return int(seed) & 0xFFFFFFFF


def _hash32(x: int) -> int:
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & 0xFFFFFFFF
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & 0xFFFFFFFF
    return x ^ (x >> 16)


def sample_uniforms(seed: int, rows: int, t: int):
    """The uniforms of step t for rows 0 .. rows-1 (csrc/vct_sample.hip, smp_uniform): the dropout kernels' counter hash at
    site SAMPLE_SITE, 24 bits each, as Python floats (exact)."""
    key = (((seed & 0xFFFFFFFF) * 0x9E3779B1) & 0xFFFFFFFF) ^ ((SAMPLE_SITE * 0x85EBCA77 + 0x165667B1) & 0xFFFFFFFF)
    k = _hash32(key)
    return [(_hash32((k + ((t * rows + r) & 0xFFFFFFFF) * 0x9E3779B1) & 0xFFFFFFFF) >> 8) / 16777216.0 for r in range(rows)]


def _sample_session(model, dec, B, N, Te, max_len, controls: bool = False) -> SampleDecodeState:
    cache = model.__dict__.setdefault("_decode_sessions", {})
    key = ("sample", B, N, Te, max_len, dec.dt) + (("ctl",) if controls else ())       # never a greedy or beam session's key
    st = cache.get(key)
    if st is None:
        if len(cache) > 3:
            cache.clear()
        st = cache[key] = SampleDecodeState(dec, B, N, Te, max_len, controls=controls)
    return st


@torch.no_grad()
def sample_decode_ids(model, feats: torch.Tensor, mask, max_len: int = 30, num_samples: int = 1, temperature: float = 1.0,
                      top_k: int = 0, top_p: float = 1.0, seed=None, use_graphs: bool = True, return_logp: bool = False,
                      sync_every: int = 4, lookahead: int = 3, controls=None):
    """Sampled decoding on the KV-cached decode step: N = num_samples captions per video drawn from the model's distribution.
    Returns ids int64 [B, N, L'] (always three dimensions, L' <= max_len); with return_logp (ids, seq_logp fp32 [B, N]), the
    sum of the drawn tokens' log-probabilities under the distribution actually sampled from (after temperature / top-k /
    nucleus), up to and including each row's end token.

    Semantics, per row (B*N independent rows, row b*N + n = sample n of video b) and step t = 1 .. max_len-1, on the step's
    logits x (bf16 on the bf16 paths): candidates = all V tokens in index order (top_k = 0) or the min(top_k, V) largest raw
    logits in rank order (value descending, ties to the smaller index; 1 <= top_k <= 64); z = float(x) / temperature in fp32,
    m = max z over the candidates, w = exp(z - m); with top_p < 1 (needs top_k >= 1: the nucleus is taken WITHIN the top-k
    candidates) only the shortest rank-order prefix whose running sum of w reaches top_p of the candidates' sum is kept; W =
    the kept sum; the token is the first kept candidate whose running sum exceeds u * W, its log-probability z - m - log W.
    u is a stateless 24-bit uniform of (seed, t, row) (sample_uniforms), so a seed reproduces a run bit for bit.  A row that
    has drawn end_id is ended: it appends pad_id, as a finished beam does.  Stop rule, layout and truncation as greedy's.
    top_k = 1 is greedy decoding up to and including each row's first end_id.

    seed=None draws one int from torch's default generator.  The settings live in a 16-byte device block that the kernels
    read, so ONE session and its captured graphs (begin + one per position) serve every seed, temperature, k and p.  The
    batch-1 block step is greedy-only: samples run on the gemv (B*N = 1), fused (bf16, 2..256 rows) or generic step.
    ValueError before any device work for an out-of-range setting.

    controls: a GenerationControls (None or a no-op: nothing changes).  The step's logits x are processed first, so the
    candidates, the draw and the log-probabilities (return_logp) are those of the CONTROLLED distribution: a banned token has
    weight 0 and is never drawn.  A session with controls is its own session, as in greedy_decode_ids."""
    _check_sample_args(num_samples, temperature, top_k, top_p)
    dec = model.cap_decoder._engine()
    controls = _resolve_controls(controls, max_len, dec.V)
    seed = _draw_seed(seed)
    B, N = _first(feats).shape[0], int(num_samples)
    st = _sample_session(model, dec, B, N, memory_len(feats), max_len, controls is not None)
    st.set_control(seed, int(top_k), float(temperature), float(top_p))
    if controls is not None:
        st.set_controls(controls)
    stop = _run_session(model, st, feats, mask, max_len, use_graphs, sync_every, lookahead, dec.sample_begin, dec.sample_step)
    ids = st.ys[:, :stop + 1].clone().view(B, N, stop + 1)
    if return_logp:
        # steps that ran past `stop` (lookahead) saw only ended rows: they added nothing
        return ids, st.seq_logp.clone().view(B, N)
    return ids


def _sample_select_ref(x: torch.Tensor, ended: torch.Tensor, u: torch.Tensor, inv_temp: float, top_k: int, top_p: float,
                       pad_id: int, delta: float):
    """Host-side selection of one step in float64 by sample_decode_ids' rule: x fp32 [M, V] -> (tokens, step log-probabilities
    fp64, undecided bool [M]: the draw was within delta of a candidate's boundary, or a nucleus cut within delta of a running
    share)."""
    M, V = x.shape
    it = torch.tensor(inv_temp, dtype=torch.float32, device=x.device)
    z = (x.float() * it).double()                                   # the product is rounded to fp32, as on the device
    if top_k == 0:
        idx = torch.arange(V, device=x.device)[None, :].expand(M, -1)
    else:
        idx = torch.sort(x.float(), dim=1, descending=True, stable=True)[1][:, :min(top_k, V)]
        z = z.gather(1, idx)
    m = z.max(1, keepdim=True)[0]
    w = torch.exp(z - m)
    cum = torch.cumsum(w, 1)
    n = cum.shape[1]
    keep = torch.full((M,), n, dtype=torch.long, device=x.device)
    cut = torch.full((M,), float("inf"), dtype=torch.float64, device=x.device)
    if top_k >= 1 and top_p < 1.0:
        p32 = float(torch.tensor(top_p, dtype=torch.float32))
        share = cum / cum[:, -1:]
        keep = (share >= p32).int().argmax(1) + 1
        cut = (share - p32).abs().min(1)[0]
    W = cum.gather(1, keep[:, None] - 1)
    kept = torch.arange(n, device=x.device)[None, :] < keep[:, None]
    hit = kept & (cum > u[:, None] * W)
    sel = torch.where(hit.any(1), hit.int().argmax(1), keep - 1)
    hi = cum.gather(1, sel[:, None]) / W
    lo = hi - w.gather(1, sel[:, None]) / W
    margin = torch.minimum(u[:, None] - lo, hi - u[:, None])[:, 0]
    tok = idx.gather(1, sel[:, None])[:, 0]
    logp = (z.gather(1, sel[:, None]) - m - torch.log(W))[:, 0]
    tok = torch.where(ended, torch.full_like(tok, pad_id), tok)
    logp = torch.where(ended, torch.zeros_like(logp), logp)
    return tok, logp, (~ended) & ((margin <= delta) | (cut <= delta))


@torch.no_grad()
def sample_decode_ids_reference_algorithm(model, feats: torch.Tensor, mask, max_len: int = 30, num_samples: int = 1,
                                          temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0, seed=None,
                                          return_logp: bool = False, delta: float = 1e-5, controls=None):
    """sample_decode_ids without the KV cache: every step re-runs the whole decoder (dec.decode_word) on the [B*N, t] histories
    and selects on the host in torch float64 by the same rule, with the same uniforms.  Returns (result as sample_decode_ids,
    undecided int64 [B, N]): per row the first step whose decision was within `delta` of a boundary -- the uniform within delta
    of an end of the chosen candidate's share of [0, 1), or the nucleus cut within delta of a running share -- and max_len where
    there is none (from that step on a test may not expect the row's ids to agree).
    controls: GenerationControls applied to every step's logits (in the dtype the decoder produced) by apply_controls_host."""
    _check_sample_args(num_samples, temperature, top_k, top_p)
    pre = model.cap_preprocessor
    model._ps.refresh_shadow()
    model._ps.refresh_lazy_transposed()
    enc, dec = model.video_encoder._engine(), model.cap_decoder._engine()
    controls = _resolve_controls(controls, max_len, dec.V)
    seed = _draw_seed(seed)
    B, N = _first(feats).shape[0], int(num_samples)
    M, Te, dev = B * N, memory_len(feats), _first(feats).device
    mem = enc.forward(feats, mask, False)
    d = mem.shape[-1]
    mem_rep = mem.reshape(B, 1, Te, d).expand(-1, N, -1, -1).reshape(M * Te, d).contiguous()
    inv_temp = float(torch.tensor(1.0 / float(temperature), dtype=torch.float32))
    hist = torch.full((M, 1), pre.start_id, dtype=torch.long, device=dev)
    ended = torch.zeros(M, dtype=torch.bool, device=dev)
    seq = torch.zeros(M, dtype=torch.float64, device=dev)
    undecided = torch.full((M,), max_len, dtype=torch.long, device=dev)
    for t in range(1, max_len):
        logits = dec.decode_word(mem_rep, M, Te, hist)
        if controls is not None:
            apply_controls_host(logits, hist, pre.end_id, controls, ended, V=dec.V)
        logits = logits.float()
        u = torch.tensor(sample_uniforms(seed, M, t), dtype=torch.float64, device=dev)
        tok, logp, und = _sample_select_ref(logits, ended, u, inv_temp, int(top_k), float(top_p), pre.pad_id, delta)
        undecided = torch.where(und & (undecided == max_len), torch.full_like(undecided, t), undecided)
        hist = torch.cat([hist, tok[:, None]], 1)
        seq += logp
        ended = ended | (tok == pre.end_id)
        if bool(ended.all()):
            break
    ids = hist.view(B, N, -1)
    res = (ids, seq.float().view(B, N)) if return_logp else ids
    return res, undecided.view(B, N)
