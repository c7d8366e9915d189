"""The decoders on the KV cache: the session cache, the token loop every session runs (captured prologue, one graph per position,
stop polling behind the launch front), and greedy / beam / sampled decoding on it."""
import torch

from ..engine import BeamDecodeState, DecodeState, SampleDecodeState, first_input as _first, memory_len, stage_inputs, static_inputs
from ..utils import capture_graph
from .controls import _resolve_controls
from .rules import _beam_finish, _beam_size, _check_sample_args, _draw_seed, _no_beam_attn


def _inputs_key(feats, mask):
    if isinstance(feats, (list, tuple)):
        return (tuple((tuple(f.shape), f.dtype) for f in feats), mask is not None)
    return (tuple(feats.shape), feats.dtype, mask is not None)


def _session(model, kind: str, key: tuple, make) -> DecodeState:
    """The model's cached session of this kind ("greedy" | "beam" | "sample") and key, built by make() when there is none.  A beam
    or sampled session carries its kind in front of its key (never a greedy session's key); more than three sessions clear the cache.
    key: the sizes, the dtype and one tag per feature whose launches the graphs bake -- a session that returns attention maps
    ("attn") or carries generation controls ("ctl") is another session, and one without is what it always was."""
    cache = model.__dict__.setdefault("_decode_sessions", {})
    key = (() if kind == "greedy" else (kind,)) + key
    st = cache.get(key)
    if st is None:
        if len(cache) > 3:
            cache.clear()
        st = cache[key] = make()
    return st


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
    B, Te, ctl = _first(feats).shape[0], memory_len(feats), controls is not None
    st = _session(model, "greedy", (B, Te, max_len, dec.dt) + (("attn",) if return_attn else ()) + (("ctl",) if ctl else ()),
                  lambda: DecodeState(dec, B, Te, max_len, return_attn=return_attn, controls=ctl))
    if ctl:
        st.set_controls(controls)
    stop = _run_session(model, st, feats, mask, max_len, use_graphs, sync_every, lookahead)
    if return_attn:
        return st.ys[:, :stop + 1].clone(), st.attn_maps[:, :, :stop].clone()
    return st.ys[:, :stop + 1].clone()


def _run_session(model, st, feats, mask, max_len, use_graphs, sync_every, lookahead) -> int:
    """The token loop of a single-model session, greedy, beam or sampled (_token_loop on this model's encoder and decoder).  Returns
    the last step to keep."""
    pre = model.cap_preprocessor
    model._ps.refresh_shadow()
    model._ps.refresh_lazy_transposed()
    enc, dec = model.video_encoder._engine(), model.cap_decoder._engine()

    def begin(fin, min_):
        dec.decode_begin(st, enc.forward(fin, min_, False), pre.start_id, pre.pad_id)

    def step(t):
        dec.decode_step(st, t, pre.end_id)
    return _token_loop(st, begin, step, lambda: model._ps.ctx.generation, feats, mask, max_len, use_graphs, sync_every, lookahead)


def _token_loop(st, begin, step, generation, feats, mask, max_len, use_graphs, sync_every, lookahead) -> int:
    """The token loop of every session: prologue, one captured graph per position, the device-side stop word polled `lookahead`
    steps behind the launch front.  begin(feats, mask): the prologue (encoder forward + the session's start) on these inputs;
    step(t): one token step; generation(): a value that moves whenever a buffer the prologue bakes has been re-allocated.  st: the
    state that owns the graphs, the stop word (all_ended_at) and the polling objects -- an ensemble's leader.  Returns the last
    step to keep."""
    on_gpu = _first(feats).device.type == "cuda"
    if on_gpu and st.poll_stream is None:
        st.poll_stream = torch.cuda.Stream(device=_first(feats).device)
        st.poll_host = torch.empty(1, dtype=torch.long).pin_memory()
        st.events = [torch.cuda.Event() for _ in range(max_len)]
    if use_graphs and on_gpu:
        # the prologue (encoder forward over the batch, cross-attention K/V of the memory for every layer, cache / flag reset:
        # ~40 launches, host-bound at 0.33 ms when issued one by one) is ONE captured graph too; the inputs go through static
        # copies.  It bakes pointers into the engines' shared grow-only buffers: re-captured whenever any of them grew.
        key = _inputs_key(feats, mask)
        bg = st.begin
        if bg is None or bg["key"] != key or bg["gen"] != generation():
            fin, min_ = static_inputs(feats, True), static_inputs(mask, True)
            begin(fin, min_)      # warm-up: allocates
            g = torch.cuda.CUDAGraph()
            with capture_graph(g):
                begin(fin, min_)
            st.begin = {"key": key, "gen": generation(), "g": g, "fin": fin, "min": min_}
        else:
            stage_inputs(bg["fin"], feats)
            if mask is not None:
                stage_inputs(bg["min"], mask)
            bg["g"].replay()
    else:
        begin(feats, mask)
    stop = max_len

    def ended_as_of(done: int) -> int:
        """all_ended_at once step `done` has run (later steps may still be in flight: the word only ever decreases to the FIRST step
        at which every row had ended, so a value read early is either max_len or final)."""
        st.events[done].synchronize()       # the HOST waits for that step (later steps stay queued on the device) ...
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
                step(t)                                    # warm-up run (allocates the step's temporaries)
                # the warm-up already wrote ys[:, t]; capture replays the same work
                g = torch.cuda.CUDAGraph()
                with capture_graph(g):
                    step(t)
                st.graphs[t] = g
            else:
                g.replay()
        else:
            step(t)
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
    K = _beam_size(beam_size, dec.V)
    controls = _resolve_controls(controls, max_len, dec.V)
    B, Te, dev, ctl = _first(feats).shape[0], memory_len(feats), _first(feats).device, controls is not None
    st = _session(model, "beam", (B, K, Te, max_len, dec.dt) + (("ctl",) if ctl else ()),
                  lambda: BeamDecodeState(dec, B, K, Te, max_len, controls=ctl))
    if ctl:
        st.set_controls(controls)
    stop = _run_session(model, st, feats, mask, max_len, use_graphs, sync_every, lookahead)
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
    B, N, Te, ctl = _first(feats).shape[0], int(num_samples), memory_len(feats), controls is not None
    st = _session(model, "sample", (B, N, Te, max_len, dec.dt) + (("ctl",) if ctl else ()),
                  lambda: SampleDecodeState(dec, B, N, Te, max_len, controls=ctl))
    st.set_sampling(seed, int(top_k), float(temperature), float(top_p))
    if ctl:
        st.set_controls(controls)
    stop = _run_session(model, st, feats, mask, max_len, use_graphs, sync_every, lookahead)
    ids = st.ys[:, :stop + 1].clone().view(B, N, stop + 1)
    if return_logp:
        # steps that ran past `stop` (lookahead) saw only ended rows: they added nothing
        return ids, st.seq_logp.clone().view(B, N)
    return ids
