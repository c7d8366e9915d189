"""The decoders without the KV cache: every step re-runs the whole decoder over the histories (dec.decode_word) and selects on the
host in torch, by the rules of the cached decoders."""
import torch

from .. import ops
from ..engine import first_input as _first, memory_len
from .controls import _resolve_controls, apply_controls_host
from .rules import _beam_finish, _beam_size, _check_sample_args, _draw_seed, _no_beam_attn, sample_uniforms


def _prologue(model, feats, mask, R: int = 1):
    """What every reference algorithm starts from: fresh shadow and lazy transposes, the encoder forward, the memory replicated
    to the R rows of every video.  Returns (decoder engine, memory [M * Te, d], M = B * R, Te, device)."""
    model._ps.refresh_shadow()
    model._ps.refresh_lazy_transposed()
    enc, dec = model.video_encoder._engine(), model.cap_decoder._engine()
    B, Te, dev = _first(feats).shape[0], memory_len(feats), _first(feats).device
    mem = enc.forward(feats, mask, False)
    if R > 1:
        d = mem.shape[-1]
        mem = mem.reshape(B, 1, Te, d).expand(-1, R, -1, -1).reshape(B * R * Te, d).contiguous()
    return dec, mem, B * R, Te, dev


@torch.no_grad()
def greedy_decode_ids_reference_algorithm(model, feats: torch.Tensor, mask, max_len: int = 30, controls=None) -> torch.Tensor:
    """controls: GenerationControls applied to every step's logits by apply_controls_host."""
    pre = model.cap_preprocessor
    controls = _resolve_controls(controls, max_len, model.cap_decoder._engine().V)
    dec, mem, B, Te, dev = _prologue(model, feats, mask)
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
    V = model.cap_decoder._engine().V
    K = _beam_size(beam_size, V)
    controls = _resolve_controls(controls, max_len, V)
    dec, mem_rep, M, Te, dev = _prologue(model, feats, mask, K)
    B = M // K
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
    controls = _resolve_controls(controls, max_len, model.cap_decoder._engine().V)
    seed = _draw_seed(seed)
    N = int(num_samples)
    dec, mem_rep, M, Te, dev = _prologue(model, feats, mask, N)
    B = M // N
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
