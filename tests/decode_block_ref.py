"""fp64 torch reference of the four block kinds of vct_decode_block (include/vct_hip.h), shared by tests/test_decode_block_gpu.py:
the batch-1 decode step of one nn.TransformerDecoderLayer cut into self-attention, cross-attention and feed-forward blocks that
each return the PARTIAL vectors of their second product (one per head / per 64 hidden units), and the generator with the greedy
token.  Written from the operation's definition, independently of the ops package and the engine: weights are taken in nn.Linear's
natural [out, in] layout, nothing is rounded, everything runs on the CPU.  `dtype` exists so that the same formulas can be
evaluated in fp32 (what a summation-order-free fp32 implementation would give against fp64)."""
import math

import torch

HD = 64          # head width and hidden units per feed-forward partial
EPS = 1e-5


def _t(x, dtype):
    return None if x is None else x.detach().to("cpu").to(dtype)


def layer_norm(x, g, b):
    mu = x.mean()
    var = ((x - mu) ** 2).mean()
    return (x - mu) / torch.sqrt(var + EPS) * g + b


def input_vector(*, embed=None, res=None, res_bias=None, part=None, ln1=None, ln2=None, dtype=torch.float64):
    """x = table[id] + pos_row  (embed = (id [1], table [V, d], pos_row [d]))  or  x = res + res_bias + sum_c part[c]
    (part [n, d]); then LayerNorm(ln1) and LayerNorm(ln2) when given (each (gamma, beta))."""
    if embed is not None:
        ids, table, pos_row = embed
        x = _t(table, dtype)[int(ids.reshape(-1)[0])] + _t(pos_row, dtype)
    else:
        x = _t(res, dtype).clone()
        if res_bias is not None:
            x = x + _t(res_bias, dtype)
        if part is not None:
            x = x + _t(part, dtype).sum(0)
    for ln in (ln1, ln2):
        if ln is not None:
            x = layer_norm(x, _t(ln[0], dtype), _t(ln[1], dtype))
    return x


def linear(x, w, b, dtype=torch.float64):
    """W x + b of one vector, W [out, in]."""
    return _t(w, dtype) @ _t(x, dtype) + _t(b, dtype)


def attention_partials(q, k, v, w_o, dtype=torch.float64):
    """One query q [d] over the keys / values k, v [Lk, d], heads of 64 columns, scale 1/sqrt(64); returns part [H, d] with
    part[h] = W_o[:, 64h:64h+64] . o_h  (w_o [d, d], natural layout) -- their sum is out_proj(attention) without its bias."""
    q, k, v, w_o = (_t(a, dtype) for a in (q, k, v, w_o))
    parts = []
    for h in range(q.shape[0] // HD):
        s = slice(h * HD, (h + 1) * HD)
        p = torch.softmax((k[:, s] @ q[s]) / math.sqrt(HD), 0)
        parts.append(w_o[:, s] @ (p @ v[:, s]))
    return torch.stack(parts)


def self_block(x, w_in, b_in, k_cache, v_cache, w_o, qkv=None, dtype=torch.float64):
    """q|k|v = W_in x + b_in ([3d]); the keys / values are the cached rows k_cache, v_cache [Lk - 1, d] followed by the fresh
    k, v.  qkv: use this [3d] instead of the projection for the attention (the projection is still returned).
    Returns (projection [3d], part [H, d])."""
    proj = linear(x, w_in, b_in, dtype)
    use = proj if qkv is None else _t(qkv, dtype)
    d = use.shape[0] // 3
    k = torch.cat([_t(k_cache, dtype).reshape(-1, d), use[None, d:2 * d]])
    v = torch.cat([_t(v_cache, dtype).reshape(-1, d), use[None, 2 * d:]])
    return proj, attention_partials(use[:d], k, v, w_o, dtype)


def cross_block(x, w_q, b_q, k_mem, v_mem, w_o, q_round=None, dtype=torch.float64):
    """q = W_q x + b_q over the memory's cached rows k_mem, v_mem [Lk, d].  q_round: a function applied to q before the
    attention (None = identity).  Returns part [H, d]."""
    q = linear(x, w_q, b_q, dtype)
    if q_round is not None:
        q = q_round(q)
    return attention_partials(q, k_mem, v_mem, w_o, dtype)


def ffn_block(x, w1, b1, w2, act, dtype=torch.float64):
    """g = act(W1 x + b1) ([ff]; act 'gelu' (erf) or 'relu'); part[c] = W2[:, 64c:64c+64] . g[64c:64c+64]  -> [ff/64, d]."""
    h = linear(x, w1, b1, dtype)
    g = 0.5 * h * (1.0 + torch.erf(h / math.sqrt(2.0))) if act == "gelu" else torch.clamp(h, min=0.0)
    w2 = _t(w2, dtype)
    return torch.stack([w2[:, c:c + HD] @ g[c:c + HD] for c in range(0, g.shape[0], HD)])


def gen_block(x, w_g, b_g, dtype=torch.float64):
    """logits = W_g x + b_g; the token is the FIRST maximal index.  Returns (logits [V], token, top-2 margin)."""
    lg = linear(x, w_g, b_g, dtype)
    tok = int((lg == lg.max()).nonzero()[0])
    top = torch.topk(lg, min(2, lg.shape[0])).values
    margin = float(top[0] - top[1]) if lg.shape[0] > 1 else float("inf")
    return lg, tok, margin
