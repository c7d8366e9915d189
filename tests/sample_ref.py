"""Numpy restatement of one sampled selection step (include/vct_hip.h, vct_sample_select; decode.sample_decode_ids): the
stateless uniforms in uint32 arithmetic and the draw in float64."""
import numpy as np

SITE = 997


def _hash32(x):
    x = x.astype(np.uint32)
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x85EBCA6B)
    x ^= x >> np.uint32(13)
    x *= np.uint32(0xC2B2AE35)
    x ^= x >> np.uint32(16)
    return x


def uniform(seed, rows, t):
    """u of step t for rows 0 .. rows-1, float64 [rows] (24 bits each: exact)."""
    with np.errstate(over="ignore"):
        seed = np.array([int(seed) & 0xFFFFFFFF], np.uint32)
        key = (seed * np.uint32(0x9E3779B1)) ^ (np.uint32(SITE) * np.uint32(0x85EBCA77) + np.uint32(0x165667B1))
        k = _hash32(key)
        idx = np.uint32(int(t) & 0xFFFFFFFF) * np.uint32(rows) + np.arange(rows, dtype=np.uint32)
        h = _hash32(k + idx * np.uint32(0x9E3779B1))
    return (h >> np.uint32(8)).astype(np.float64) / 16777216.0


def candidates(x_row, top_k):
    """Candidate columns of one row in candidate order: every column (top_k = 0), else the min(top_k, V) largest raw logits,
    value descending, ties to the smaller index."""
    V = x_row.shape[0]
    if top_k == 0:
        return np.arange(V)
    return np.argsort(-x_row.astype(np.float64), kind="stable")[:min(top_k, V)]


def select_step(x, ended, seed, t, inv_temp, top_k, top_p, pad, end):
    """x fp32 [rows, V] (already rounded to the logits' dtype), ended bool [rows].  Returns (tokens int64, step_logp float64,
    new ended, margin, cut): margin = min(u - lo, hi - u) with [lo, hi) the chosen candidate's share of [0, 1); cut = the
    distance of top_p from the nearest running share (inf without a nucleus).  Ended rows: pad, 0, inf, inf."""
    rows, V = x.shape
    u = uniform(seed, rows, t)
    it = np.float32(inv_temp)
    p32 = float(np.float32(top_p))
    tok = np.full(rows, pad, np.int64)
    logp = np.zeros(rows, np.float64)
    margin = np.full(rows, np.inf)
    cut = np.full(rows, np.inf)
    for r in range(rows):
        if ended[r]:
            continue
        idx = candidates(x[r], top_k)
        z = (x[r, idx].astype(np.float32) * it).astype(np.float64)        # the product is rounded to fp32
        m = z.max()
        w = np.exp(z - m)
        cum = np.cumsum(w)
        keep = idx.size
        if top_k >= 1 and p32 < 1.0:
            share = cum / cum[-1]
            keep = int(np.argmax(share >= p32)) + 1
            cut[r] = np.abs(share - p32).min()
        W = cum[keep - 1]
        hit = np.flatnonzero(cum[:keep] > u[r] * W)
        sel = int(hit[0]) if hit.size else keep - 1
        hi = cum[sel] / W
        lo = (cum[sel] - w[sel]) / W
        margin[r] = min(u[r] - lo, hi - u[r])
        tok[r] = idx[sel]
        logp[r] = z[sel] - m - np.log(W)
    return tok, logp, ended | (tok == end), margin, cut


def neighbours(x_row, top_k, token):
    """The candidates next to `token` in candidate order (what a draw within delta of a boundary may give instead)."""
    idx = candidates(x_row, top_k)
    pos = int(np.flatnonzero(idx == token)[0])
    return {int(idx[p]) for p in (pos - 1, pos + 1) if 0 <= p < idx.size}
