"""numpy beam search on the oracle (vct_oracle.decode_word / mm_encoder_forward): the semantics of decode.beam_decode_ids,
restated independently of the package.  Fixed-width beams, finished hypotheses frozen; see decode.beam_decode_ids."""
import numpy as np

import vct_oracle as O


def select(vals: np.ndarray, valid: np.ndarray, K: int):
    """One video's selection: vals / valid [K*V] -> (flat indices [K], values [K], K-th minus (K+1)-th value or inf).
    Valid entries first, then value descending, then flat index ascending."""
    order = np.lexsort((np.arange(vals.size), -vals.astype(np.float64), ~valid))
    top = order[:K]
    margin = np.inf
    if vals.size > K and valid[order[K]] and np.isfinite(vals[order[K]]):
        margin = float(vals[order[K - 1]]) - float(vals[order[K]])
    return top, vals[top], margin


def select_step(logits: np.ndarray, scores: np.ndarray, finished: np.ndarray, K: int, pad_id: int, end_id: int):
    """One step for every video.  logits [B*K, V] (any float dtype, read as fp32), scores fp32 [B*K], finished bool [B*K] ->
    (parent rows int32 [B*K], tokens int64 [B*K], new scores fp32 [B*K], new finished bool [B*K], min margin)."""
    x = logits.astype(np.float32)
    M, V = x.shape
    B = M // K
    m = x.max(1, keepdims=True).astype(np.float64)
    lse = (m[:, 0] + np.log(np.exp(x.astype(np.float64) - m).sum(1))).astype(np.float32)
    logp = (x - lse[:, None]).astype(np.float32)
    vals = (scores.astype(np.float32)[:, None] + logp).astype(np.float32)
    valid = np.repeat(~finished[:, None], V, 1)
    vals[finished] = -np.inf
    vals[finished, pad_id] = scores[finished]
    valid[finished, pad_id] = True
    parent = np.empty(M, np.int32)
    tok = np.empty(M, np.int64)
    new_s = np.empty(M, np.float32)
    margin = np.inf
    for b in range(B):
        flat, val, mg = select(vals[b * K:(b + 1) * K].reshape(-1), valid[b * K:(b + 1) * K].reshape(-1), K)
        margin = min(margin, mg)
        parent[b * K:(b + 1) * K] = b * K + flat // V
        tok[b * K:(b + 1) * K] = flat % V
        new_s[b * K:(b + 1) * K] = val
    new_f = finished[parent] | (tok == end_id)
    return parent, tok, new_s, new_f, margin


def finish(hist: np.ndarray, scores: np.ndarray, B: int, K: int, end_id: int, alpha: float):
    """-> ids [B, K, L'] and final scores fp32 [B, K], each video's slots sorted by s / n^alpha (descending, ties: lower slot)."""
    gen = hist[:, 1:] == end_id
    n = np.where(gen.any(1), gen.argmax(1) + 1, gen.shape[1]).astype(np.float32)
    final = (scores.astype(np.float32) / np.power(n, np.float32(alpha))).astype(np.float32).reshape(B, K)
    order = np.argsort(-final, axis=1, kind="stable")
    ids = np.take_along_axis(hist.reshape(B, K, -1), order[:, :, None], 1)
    return ids, np.take_along_axis(final, order, 1)


def beam_search(p, cfg, feats, mask, K: int, max_len: int = 30, alpha: float = 1.0, start_id=101, end_id=102, pad_id=0):
    """-> (ids [B, K, L'] sorted best first, final scores [B, K], smallest top-K margin over every video and step)."""
    mem = O.mm_encoder_forward(p, cfg, feats, mask)[0]
    B = feats.shape[0]
    M = B * K
    mem_rep = np.repeat(mem, K, 0)
    hist = np.full((M, 1), start_id, np.int64)
    s = np.full(M, -np.inf, np.float32)
    s[::K] = 0.0
    fin = np.zeros(M, bool)
    margin = np.inf
    for _ in range(max_len - 1):
        logits = O.decode_word(p, cfg, mem_rep, hist)
        parent, tok, s, fin, mg = select_step(logits, s, fin, K, pad_id, end_id)
        margin = min(margin, mg)
        hist = np.concatenate([hist[parent], tok[:, None]], 1)
        if fin.all():
            break
    ids, final = finish(hist, s, B, K, end_id, alpha)
    return ids, final, margin
