"""Ensemble decoding: several models behind one greedy / beam / sampled session on the KV cache.

At every step each member runs its own decode step on its own caches, vct_ensemble_combine turns the members' logits into ONE
fp32 row of combined log-probabilities per decode row, and the session's controls and selection run once, on that row (a row of
log-probabilities is a valid logits row, so the selection kernels are the single-model ones).

    mode "prob"     p(v) = sum_m w_m p_m(v), the arithmetic mean of the members' next-token distributions
    mode "logprob"  log p(v) = sum_m w_m log p_m(v) (+ const), the geometric mean; the selection stages renormalise

Session layout: a LEADER state of the requested kind that owns the id matrix, the end / beam / sampling bookkeeping, the
controls, the selection, the captured graphs and the combined logits -- but no decoder, no cache and no memory -- and one MEMBER
state per model that owns that model's caches and step temporaries and aliases the leader's token and bookkeeping tensors.  A
member carries no controls and selects nothing: its step ends with its logits in last_logits.  The generation controls run after
the combination because they are rules on the distribution that is sampled from (a banned id must have probability zero in the
ensemble, a repetition penalty must scale the ensemble's score once, not every member's before an average that would dilute it
by the members' weights)."""
import math

import torch

from .. import ops
from ..engine import BeamDecodeState, DecodeState, SampleDecodeState, first_input as _first, memory_len
from ..engine.decode_step import _finish_step
from .cached import _session, _token_loop
from .controls import _resolve_controls
from .rules import _beam_finish, _beam_size, _check_sample_args, _draw_seed

ENSEMBLE_MAX = 8
MODES = {"prob": "prob", "logprob": "logp"}


def normalise_weights(weights, n: int):
    """The n member weights as the kernel reads them: non-negative, summing to 1, padded with zeros to ENSEMBLE_MAX floats.
    None = uniform.  ValueError for a wrong length, a negative or non-finite weight, or weights that sum to zero."""
    if weights is None:
        weights = [1.0] * n
    w = [float(x) for x in weights]
    if len(w) != n:
        raise ValueError(f"ensemble: {len(w)} weights for {n} members")
    if any(not math.isfinite(x) or x < 0.0 for x in w):
        raise ValueError(f"ensemble: weights must be finite and >= 0, got {w}")
    total = math.fsum(w)
    if not total > 0.0:
        raise ValueError("ensemble: the weights sum to zero")
    return [x / total for x in w] + [0.0] * (ENSEMBLE_MAX - n)


class _LeaderEngine:
    """What a session state asks of its engine, for the leader: the vocabulary and the device of the members, fp32 logits, and NO
    layers -- so the state allocates no cache and its start() projects no memory."""

    def __init__(self, eng):
        self.cfg = dict(eng.cfg, layers=0)
        self.dt, self.dev, self.ps, self.V, self.Vp = torch.float32, eng.dev, eng.ps, eng.V, eng.Vp


class _BeamLeader(BeamDecodeState):
    """The beam leader's selection: vct_beam_select once, on the combined row, then every MEMBER's cache follows the parents."""

    members = ()

    def select(self, eng, logits, t, end_id):
        ops.beam_select(logits, self.Bv, self.K, self.scores, self.finished, self.parents[t], self.ys[:, t], end_id, self.pad_id,
                        self.fin_count[t:t + 1], self.all_ended_at, t, self.sel_ws, cols=eng.V)
        for dec, st in self.members:
            ops.beam_reorder(st.kv_layers[t % 2], st.kv_layers[(t + 1) % 2], self.parents[t], self.B, self.Lmax, dec.cfg["d"], t)


def _no_select(eng, logits, t, end_id):
    return None


def _make_session(kind, engines, rows_args, Te, max_len, ctl):
    """Leader + one member state per decoder engine.  rows_args: (B,) greedy, (B, K) beam, (B, N) sampled."""
    lead_eng = _LeaderEngine(engines[0])
    cls = {"greedy": DecodeState, "beam": BeamDecodeState, "sample": SampleDecodeState}[kind]
    lead_cls = _BeamLeader if kind == "beam" else cls
    leader = lead_cls(lead_eng, *rows_args, Te, max_len, controls=ctl)
    leader.mem_rep = None                       # (the leader reads no memory)
    leader.fused_select = False
    members = []
    for dec in engines:
        st = cls(dec, *rows_args, Te, max_len)
        st.ys, st.ended = leader.ys, leader.ended
        if kind == "beam":
            st.parents, st.finished = leader.parents, leader.finished
        st.fused_select = False                 # never the batch-1 block step: it selects inside its generator launch
        st.select = _no_select                  # _finish_step leaves the member's logits in last_logits and stops there
        members.append((dec, st))
    leader.members = members
    leader.lead_eng = lead_eng
    leader.logits = torch.zeros(leader.B, lead_eng.Vp, dtype=torch.float32, device=lead_eng.dev)
    return leader


class Ensemble:
    """Several MMT4Caption models decoded as one: Ensemble(models, weights=None, mode="prob").  weights: one non-negative number
    per model (normalised to sum 1; None = uniform); mode "prob" averages the members' probabilities, "logprob" their
    log-probabilities.  Members may differ in width, depth, encoder type and compute dtype; they share the device, the vocabulary
    (size, start / end / pad ids) and the number of feature streams.  The *_decode_ids methods take the arguments of the module
    functions of decode/cached.py behind (feats, masks) -- per-stream lists, as MMT4Caption's methods take them -- and the string
    methods those of MMT4Caption's; there is no kv_cache argument (an ensemble always runs on the KV cache).  Strings come from
    the first member's preprocessor."""

    def __init__(self, models, weights=None, mode: str = "prob"):
        models = list(models)
        if not 1 <= len(models) <= ENSEMBLE_MAX:
            raise ValueError(f"ensemble: {len(models)} members (1..{ENSEMBLE_MAX})")
        if mode not in MODES:
            raise ValueError(f"ensemble: mode {mode!r} (one of {sorted(MODES)})")
        first = models[0]
        pre = first.cap_preprocessor
        for i, m in enumerate(models[1:], 1):
            mine, theirs = torch.device(first.device), torch.device(m.device)
            if theirs.type != mine.type or (None not in (mine.index, theirs.index) and mine.index != theirs.index):
                raise ValueError(f"ensemble: member {i} is on {m.device}, member 0 on {first.device}")
            p = m.cap_preprocessor
            V, V0 = m.cap_decoder.cfg["vocab"], first.cap_decoder.cfg["vocab"]
            if V != V0:
                raise ValueError(f"ensemble: member {i} has vocabulary size {V}, member 0 {V0}")
            if (p.start_id, p.end_id, p.pad_id) != (pre.start_id, pre.end_id, pre.pad_id):
                raise ValueError(f"ensemble: member {i} has (start, end, pad) ids {(p.start_id, p.end_id, p.pad_id)}, member 0 "
                                 f"{(pre.start_id, pre.end_id, pre.pad_id)}")
            if m.video_encoder.num_modal != first.video_encoder.num_modal:
                raise ValueError(f"ensemble: member {i} takes {m.video_encoder.num_modal} feature streams, member 0 "
                                 f"{first.video_encoder.num_modal}")
        w = normalise_weights(weights, len(models))
        self.models, self.mode = models, mode
        self.weights = w[:len(models)]
        self._w = torch.tensor(w, dtype=torch.float32).to(first.device)     # the 32 bytes vct_ensemble_combine reads on the device

    # ---- the surface evaluate.py uses of a model ---------------------------------------------------------------------------
    @property
    def device(self):
        return self.models[0].device

    @property
    def cap_preprocessor(self):
        return self.models[0].cap_preprocessor

    def eval(self):
        for m in self.models:
            m.eval()
        return self

    def _ids_to_captions(self, ys):
        return self.models[0]._ids_to_captions(ys)

    def set_weights(self, weights):
        """New member weights for every session of this ensemble: one 32-byte host -> device copy, no recapture."""
        w = normalise_weights(weights, len(self.models))
        self.weights = w[:len(self.models)]
        self._w.copy_(torch.tensor(w, dtype=torch.float32))

    # ---- sessions ---------------------------------------------------------------------------------------------------------------
    def _engines(self):
        return [m.cap_decoder._engine() for m in self.models]

    def _run(self, kind, rows_args, feats, mask, max_len, use_graphs, sync_every, lookahead, controls, prepare=None):
        """The leader state after a run of this kind on these inputs, and the last step to keep."""
        pre = self.cap_preprocessor
        was = [m.training for m in self.models]
        self.eval()
        try:
            feats, mask = self.models[0]._video_inputs(feats, mask)
            for m in self.models:
                if not m._ps.intact():
                    m._build_flat()
                m._ps.refresh_shadow()
                m._ps.refresh_lazy_transposed()
            decs = self._engines()
            encs = [m.video_encoder._engine() for m in self.models]
            controls = _resolve_controls(controls, max_len, decs[0].V)
            ctl = controls is not None
            rows_args = (_first(feats).shape[0],) + tuple(rows_args)
            Te = memory_len(feats)
            key = rows_args + (Te, max_len, tuple(d.dt for d in decs)) + (("ctl",) if ctl else ())
            leader = _session(self, kind, key, lambda: _make_session(kind, decs, rows_args, Te, max_len, ctl))
            if prepare is not None:
                prepare(leader)
            if ctl:
                leader.set_controls(controls)
            lead_eng, members, w, mode = leader.lead_eng, leader.members, self._w, MODES[self.mode]

            def begin(fin, min_):
                for enc, (dec, st) in zip(encs, members):
                    dec.decode_begin(st, enc.forward(fin, min_, False), pre.start_id, pre.pad_id)
                leader.start(lead_eng, None, pre.start_id, pre.pad_id)

            def step(t):
                for dec, st in members:
                    dec.decode_step(st, t, pre.end_id)
                ops.ensemble_combine([st.last_logits for _, st in members], w, leader.logits, mode, cols=lead_eng.V)
                _finish_step(lead_eng, leader, leader.logits, t, pre.end_id)
            stop = _token_loop(leader, begin, step, lambda: tuple(m._ps.ctx.generation for m in self.models), feats, mask, max_len,
                               use_graphs, sync_every, lookahead)
            return leader, stop
        finally:
            for m, t in zip(self.models, was):
                m.train(t)

    @staticmethod
    def _no_attn(return_attn):
        if return_attn:
            raise ValueError("return_attn is not available from an ensemble: the attention maps are each member's own")

    # ---- ids ----------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def greedy_decode_ids(self, video_feat, video_masks=None, max_len: int = 30, use_graphs: bool = True, sync_every: int = 4,
                          lookahead: int = 3, return_attn: bool = False, controls=None):
        """decode.greedy_decode_ids on the combined distribution: ys int64 [B, <= max_len]."""
        self._no_attn(return_attn)
        st, stop = self._run("greedy", (), video_feat, video_masks, max_len, use_graphs, sync_every, lookahead, controls)
        return st.ys[:, :stop + 1].clone()

    @torch.no_grad()
    def beam_decode_ids(self, video_feat, video_masks=None, beam_size: int = 5, max_len: int = 30, length_penalty: float = 1.0,
                        use_graphs: bool = True, return_all: bool = False, sync_every: int = 4, lookahead: int = 3,
                        return_attn: bool = False, controls=None):
        """decode.beam_decode_ids on the combined distribution: the scores are sums of log-probabilities of the combined,
        controlled distribution."""
        self._no_attn(return_attn)
        pre = self.cap_preprocessor
        K = _beam_size(beam_size, self.models[0].cap_decoder.cfg["vocab"])
        st, stop = self._run("beam", (K,), video_feat, video_masks, max_len, use_graphs, sync_every, lookahead, controls)
        B, M, dev = st.Bv, st.B, st.ys.device
        ids = torch.empty(M, stop + 1, dtype=torch.long, device=dev)
        ids[:, 0] = pre.start_id
        r = torch.arange(M, device=dev)
        for t in range(stop, 0, -1):
            ids[:, t] = st.ys[r, t]
            r = st.parents[t].long()[r]
        return _beam_finish(ids, st.scores.clone(), B, K, pre.end_id, length_penalty, return_all)

    @torch.no_grad()
    def sample_decode_ids(self, video_feat, video_masks=None, max_len: int = 30, num_samples: int = 1, temperature: float = 1.0,
                          top_k: int = 0, top_p: float = 1.0, seed=None, use_graphs: bool = True, return_logp: bool = False,
                          sync_every: int = 4, lookahead: int = 3, controls=None):
        """decode.sample_decode_ids on the combined distribution: ids int64 [B, N, L'] (return_logp: + seq_logp fp32 [B, N], the
        log-probabilities under the combined, controlled distribution that was sampled from)."""
        _check_sample_args(num_samples, temperature, top_k, top_p)
        seed, N = _draw_seed(seed), int(num_samples)
        st, stop = self._run("sample", (N,), video_feat, video_masks, max_len, use_graphs, sync_every, lookahead, controls,
                             prepare=lambda s: s.set_sampling(seed, int(top_k), float(temperature), float(top_p)))
        ids = st.ys[:, :stop + 1].clone().view(st.Bv, N, stop + 1)
        if return_logp:
            return ids, st.seq_logp.clone().view(st.Bv, N)
        return ids

    # ---- strings ------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def greedy_decode(self, video_feat, video_masks=None, max_len: int = 30, return_attn: bool = False, controls=None):
        return self._ids_to_captions(self.greedy_decode_ids(video_feat, video_masks, max_len, return_attn=return_attn, controls=controls))

    @torch.no_grad()
    def beam_decode(self, video_feat, video_masks=None, beam_size: int = 5, max_len: int = 30, length_penalty: float = 1.0,
                    return_attn: bool = False, controls=None):
        return self._ids_to_captions(self.beam_decode_ids(video_feat, video_masks, beam_size, max_len, length_penalty,
                                                          return_attn=return_attn, controls=controls))

    @torch.no_grad()
    def sample_decode(self, video_feat, video_masks=None, num_samples: int = 1, max_len: int = 30, temperature: float = 1.0,
                      top_k: int = 0, top_p: float = 1.0, seed=None, controls=None):
        ids = self.sample_decode_ids(video_feat, video_masks, max_len, num_samples, temperature, top_k, top_p, seed, controls=controls)
        B, N = ids.shape[0], ids.shape[1]
        flat = self._ids_to_captions(ids.reshape(B * N, -1))
        return [flat[b * N:(b + 1) * N] for b in range(B)]
