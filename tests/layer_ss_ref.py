"""fp64 torch reference (CPU) of the sample-stationary stack kernels (include/vct_hip.h: vct_layer_ss_fwd, vct_layer_ss_bwd, vct_ss_pack),
shared by tests/test_layer_ss_ref_cpu.py (which checks THIS file against torch.nn and the oracle) and tests/test_layer_ss_kernels_gpu.py.
Written from the operations' definitions: one post-norm nn.TransformerEncoderLayer / nn.TransformerDecoderLayer (eps 1e-5, gelu (erf) or
relu, 8 heads of 64, d = 512), the stack-final LayerNorm, the two prologues, the hand-written gradients of the encoder layer, the dropout
counter hash of csrc/vct_common.h and the stream order of the packed weights.  Weights are taken in nn.Linear's [out, in] layout.

Two modes (argument `got` of layer_fwd / stack_fwd):
  chain mode (got = None)   fp64 from the stack input all the way through, nothing rounded: the end-to-end reference;
  step mode  (got = saved tensors of the kernel)   every saved tensor is recomputed in fp64 from the operand the KERNEL stored one
             product earlier.  The kernel completes each saved tensor in an LDS panel (bf16) and copies that panel to HBM, and the next
             product reads the same panel: the stored tensor IS the next operand, so one product is judged at a time, without drift.

Operand form mirrored in step mode, tensor by tensor (read in csrc/vct_layer_ss.hip and csrc/vct_layer_ss_core.h):
  qkv            layer input as stored: x (layers[0].x, or the x the prologue stored) / the previous layer's n3.y (panel R0 = YP; the
                 second launch of a deep stack re-reads layers[base-1].n3.y from HBM: the same values)
  o              q | k | v as stored (panel R1A, ss_attn_wave).  The probabilities continue in fp32 and are rounded to bf16 for the P V
                 product (pack_p): NOT mirrored, covered by the bf16 tolerance.  A fully masked row gives o = 0 (inv = 0)
  a              o as stored (panel R0)
  n1.{y,mean,rstd}   s = a AS STORED (epi_ln: "the norm is built on it") * dropout + the layer input as stored (res registers from R0);
                 statistics and y in fp32 on s
  cq             n1.y as stored (R1B);   ckv   mem as given (panel RM);   co   cq, ckv as stored;   ca   co as stored (R1A)
  n2.*           ca as stored * dropout + n1.y as stored
  hpre           n1.y (encoder) / n2.y (decoder) as stored (panel FIN)
  h              hpre AS STORED (the header's text; ffn_tile reads the packed bf16 hpk): act(hpre) * dropout
  f              h as stored (panels HP0 / HP1), ONE fp32 accumulation over all of ff (facc rides through the chunk loop)
  n3.*           f as stored * dropout + the feed-forward input as stored;   nf.*   n3.y as stored (epi_ln: "a second norm reads the
                 rows as STORED")
  x (pro = 1)    u = bf16(feats) W_u^T + b_u is ROUNDED TO bf16 in flight (the kernel mirrors what the unfused path stores) before the
                 mean over the frames and before + PE': frontend(round_u=True) mirrors exactly that;  x_in = bf16(feats), bit for bit
  x (pro = 2)    (table[id] + pos) * dropout, fp32 in flight, nothing stored in between
Backward (csrc/vct_layer_ss_bwd.hip): the gradient rows stay in fp32 registers from dy to dx (gy); only d hpre is one product away
from a stored operand (d f, panel S3 = what is stored): dhpre_step mirrors it.  Everything else is compared in chain mode."""
import math

import numpy as np
import torch

D, H, HD, EPS = 512, 8, 64, 1e-5
SS_CHUNK = 32768          # bf16 elements per 64-KiB chunk of a packed weight stream
F64 = torch.float64


def _d(x):
    return None if x is None else x.to("cpu").to(F64)


def bf16(x):
    """Round to bf16 (nearest even), back in fp64."""
    return x.detach().to("cpu").to(torch.float32).to(torch.bfloat16).to(F64)


# ---- dropout: the counter hash of csrc/vct_common.h (make_dropout, hash32, drop_mult) -------------------------------------------------
_M32 = np.uint64(0xFFFFFFFF)


def _hash32(x):
    x = x.astype(np.uint64)
    x ^= x >> np.uint64(16); x = (x * np.uint64(0x85EBCA6B)) & _M32
    x ^= x >> np.uint64(13); x = (x * np.uint64(0xC2B2AE35)) & _M32
    x ^= x >> np.uint64(16)
    return x


def drop_mult(seed, site, p, idx):
    """Multiplier (0 or 1 / (1 - p), fp32 as the kernels hold it) of the elements `idx` (any integer array; counters wrap at 2^32) of
    dropout site `site`: key = seed * 0x9E3779B1 ^ (site * 0x85EBCA77 + 0x165667B1); one hash per element PAIR, low / high 16-bit field
    for the even / odd element; dropped when the field < p * 65536 + 0.5 (truncated, at most 65535)."""
    idx = np.asarray(idx).astype(np.uint64) & _M32
    if seed is None or p <= 0.0:
        return np.ones(idx.shape)
    key = ((np.uint64(seed) * np.uint64(0x9E3779B1)) & _M32) ^ ((np.uint64(site) * np.uint64(0x85EBCA77) + np.uint64(0x165667B1)) & _M32)
    thresh = np.uint64(int(min(np.float32(p) * np.float32(65536.0) + np.float32(0.5), np.float32(65535.0))))
    scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
    h = _hash32((((idx >> np.uint64(1)) * np.uint64(0x9E3779B1)) & _M32) ^ key)
    field = np.where(idx & np.uint64(1), h >> np.uint64(16), h & np.uint64(0xFFFF))
    return np.where(field < thresh, 0.0, scale)


def row_drop(seed, site, p, M, ncols):
    """Residual / feed-forward / embedding sites: element (global row r, column c) of an [M, ncols] tensor has counter r * ncols + c."""
    idx = np.arange(M, dtype=np.uint64)[:, None] * np.uint64(ncols) + np.arange(ncols, dtype=np.uint64)[None]
    return torch.from_numpy(drop_mult(seed, site, p, idx))


def attn_drop(seed, site, p, B, Lq, Lk):
    """Attention probabilities: counter ((b * 8 + head) * Lq + query) * Lk + key -> [B, H, Lq, Lk]."""
    idx = np.arange(B * H * Lq * Lk, dtype=np.uint64).reshape(B, H, Lq, Lk)
    return torch.from_numpy(drop_mult(seed, site, p, idx))


# ---- primitive operations -----------------------------------------------------------------------------------------------------------
def linear(a, w, b):
    """(a W^T + b,  sum_k |a_k w_k| + |b|): the value and the magnitude sum the element-wise fp32 bound is built from."""
    a, w, b = _d(a), _d(w), _d(b)
    return a @ w.t() + b, a.detach().abs() @ w.detach().abs().t() + b.detach().abs()


def act_fn(name, x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0))) if name == "gelu" else torch.clamp(x, min=0.0)


def dact_fn(name, x):
    if name == "gelu":
        return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    return (x > 0).to(F64)


def key_mask(B, L, key_pad=None, shift=0, key_ids=None, pad_id=0):
    """vct_attn_desc's key padding as one bool [B, L] (True = masked): key_pad [B, L - shift] with the first `shift` keys never padded,
    or key_ids [B, >= L] compared with pad_id."""
    if key_ids is not None:
        return key_ids.cpu()[:, :L] == pad_id
    if key_pad is None:
        return None
    m = torch.zeros(B, L, dtype=torch.bool)
    m[:, shift:] = key_pad.cpu().reshape(B, L - shift) != 0
    return m


def softmax_masked(q, k, B, Lq, Lk, causal, kpm):
    """Probabilities [B, H, Lq, Lk] of q [B*Lq, 512], k [B*Lk, 512]; a fully masked row is ALL ZERO (the project's convention)."""
    qh = q.view(B, Lq, H, HD).transpose(1, 2)
    kh = k.view(B, Lk, H, HD).transpose(1, 2)
    s = qh @ kh.transpose(-1, -2) / math.sqrt(HD)
    masked = torch.zeros(B, 1, Lq, Lk, dtype=torch.bool)
    if causal:
        masked = masked | torch.triu(torch.ones(Lq, Lk, dtype=torch.bool), 1)
    if kpm is not None:
        masked = masked | kpm[:, None, None, :]
    s = s.masked_fill(masked, float("-inf"))
    m = s.amax(-1, keepdim=True)
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    return torch.where(l > 0, e / torch.where(l > 0, l, torch.ones_like(l)), torch.zeros_like(e))


def attention(q, k, v, B, Lq, Lk, causal, kpm, mult):
    p = softmax_masked(q, k, B, Lq, Lk, causal, kpm) * mult
    vh = v.view(B, Lk, H, HD).transpose(1, 2)
    return (p @ vh).transpose(1, 2).reshape(B * Lq, D)


def add_ln(xs, res, mult, g, b):
    """LayerNorm(res + xs * mult) -> (y, mean, rstd, sum_c |s|)."""
    s = xs * mult + (0.0 if res is None else res)
    mean = s.mean(1)
    c = s - mean[:, None]
    rstd = 1.0 / torch.sqrt((c * c).mean(1) + EPS)
    return c * rstd[:, None] * _d(g) + _d(b), mean, rstd, s.detach().abs().sum(1)


class Cfg:
    """Shape, masks and dropout of one stack: B samples of L rows (Lm memory rows: decoder), kpm = key_mask(...) or None."""

    def __init__(self, B, L, ff, act="gelu", Lm=0, mem=None, causal=False, kpm=None, seed=None, p=0.0):
        self.B, self.L, self.ff, self.act, self.Lm, self.mem = B, L, ff, act, Lm, _d(mem)
        self.causal, self.kpm, self.seed, self.p = causal, kpm, seed, p


# ---- forward ----------------------------------------------------------------------------------------------------------------------------
def layer_fwd(x, w, c, sites, got=None, final=None):
    """One layer on x [B*L, 512].  w: w_in, b_in, w_o, b_o, [c_in, cb_in, c_o, cb_o, n2,] w1, b1, w2, b2, n1, n3 (norms = (gamma, beta));
    sites = (self-attention probabilities, norm1, cross-attention probabilities, norm2, feed-forward, last norm); final = (gamma, beta)
    of the stack-final norm behind this layer.  Returns (out, S): every saved tensor by name, and for the pure products the magnitude
    sums (S[name]), for the means sum_c |s| (S['n1.mean'] ...).  got: see the module docstring."""
    B, L, M = c.B, c.L, c.B * c.L
    x = _d(x)
    out, S = {}, {}

    def use(name):
        return out[name] if got is None else _d(got[name])

    def norm(tag, xs, res, site, gb):
        mult = 1.0 if site is None else row_drop(c.seed, site, c.p, M, D)
        out[tag + ".y"], out[tag + ".mean"], out[tag + ".rstd"], S[tag + ".mean"] = add_ln(xs, res, mult, *gb)

    out["qkv"], S["qkv"] = linear(x, w["w_in"], w["b_in"])
    qkv = use("qkv")
    out["o"] = attention(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], B, L, L, c.causal, c.kpm, attn_drop(c.seed, sites[0], c.p, B, L, L))
    out["a"], S["a"] = linear(use("o"), w["w_o"], w["b_o"])
    norm("n1", use("a"), x, sites[1], w["n1"])
    fin = use("n1.y")
    if c.Lm:
        out["cq"], S["cq"] = linear(fin, w["c_in"][:D], w["cb_in"][:D])
        out["ckv"], S["ckv"] = linear(c.mem, w["c_in"][D:], w["cb_in"][D:])
        ckv = use("ckv")
        out["co"] = attention(use("cq"), ckv[:, :D], ckv[:, D:], B, L, c.Lm, False, None, attn_drop(c.seed, sites[2], c.p, B, L, c.Lm))
        out["ca"], S["ca"] = linear(use("co"), w["c_o"], w["cb_o"])
        norm("n2", use("ca"), fin, sites[3], w["n2"])
        fin = use("n2.y")
    out["hpre"], S["hpre"] = linear(fin, w["w1"], w["b1"])
    out["h"] = act_fn(c.act, use("hpre")) * row_drop(c.seed, sites[4], c.p, M, c.ff)
    out["f"], S["f"] = linear(use("h"), w["w2"], w["b2"])
    norm("n3", use("f"), fin, sites[5], w["n3"])
    if final is not None:
        norm("nf", use("n3.y"), None, None, final)
    return out, S


def stack_fwd(x, layers, c, sites, final=None, got=None):
    """The layers in turn; got = list of the kernel's saved tensors per layer (step mode: layer l > 0 reads got[l-1]['n3.y']).  final
    belongs to the last layer.  Returns [(out, S)] per layer."""
    res, x = [], _d(x)
    for l, w in enumerate(layers):
        res.append(layer_fwd(x, w, c, sites[l], None if got is None else got[l], final if l == len(layers) - 1 else None))
        x = res[-1][0]["n3.y"] if got is None else _d(got[l]["n3.y"])
    return res


def frontend(feats, w_u, b_u, pe_rows, B, T, round_u=False):
    """pro = 1: u = bf16(feats) W_u^T + b_u; row 0 = mean over ALL T frames of u + PE'[0], row t + 1 = u_t + PE'[t + 1]
    (MMEncoder.py:246-271).  round_u: u rounded to bf16 first, as the kernel holds it.  Returns (x [B*(T+1), 512], x_in [B*T, 512])."""
    x_in = bf16(feats) if feats.dtype != F64 else _d(feats)
    u = (x_in @ _d(w_u).t() + _d(b_u))
    if round_u:
        u = bf16(u)
    u = u.view(B, T, D)
    z = torch.cat([u.mean(1, keepdim=True), u], 1) + _d(pe_rows)[None, :T + 1]
    return z.reshape(B * (T + 1), D), x_in


def embed(ids, table, pos, B, L, seed=None, site=0, p=0.0):
    """pro = 2: x = dropout(table[ids[b, s]] + pos[s]) (CapDecoder.py:48, Embedding.py:23-25) -> [B*L, 512]."""
    e = _d(table)[ids.cpu()[:, :L]] + _d(pos)[None, :L]
    return e.reshape(B * L, D) * row_drop(seed, site, p, B * L, D)


# ---- backward of the encoder layer (hand-written, on the SAVED forward tensors as the kernel reads them) ----------------------------------
def ln_bwd(dy, xs, res, mult, g, mean, rstd, B):
    """z = res + xs * mult, h = (z - mean) rstd (saved statistics); ds = rstd (dy g - mean_c(dy g) - h mean_c(dy g h)).
    Returns (ds, ds * mult, per-sample partial rows [B, 2, 512] = (sum_rows dy h | sum_rows dy))."""
    z = xs * mult + (0.0 if res is None else res)
    h = (z - mean[:, None]) * rstd[:, None]
    dh = dy * _d(g)
    ds = rstd[:, None] * (dh - dh.mean(1, keepdim=True) - h * (dh * h).mean(1, keepdim=True))
    part = torch.stack([(dy * h).view(B, -1, D).sum(1), dy.view(B, -1, D).sum(1)], 1)
    return ds, ds * mult, part


def attention_bwd(do, qkv, B, L, causal, kpm, mult):
    q, k, v = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
    p = softmax_masked(q, k, B, L, L, causal, kpm)
    heads = lambda t: t.view(B, L, H, HD).transpose(1, 2)
    qh, kh, vh, doh = heads(q), heads(k), heads(v), heads(do)
    dp = (doh @ vh.transpose(-1, -2)) * mult
    dv = (p * mult).transpose(-1, -2) @ doh
    dS = p * (dp - (dp * p).sum(-1, keepdim=True)) / math.sqrt(HD)
    dq, dk = dS @ kh, dS.transpose(-1, -2) @ qh
    flat = lambda t: t.transpose(1, 2).reshape(B * L, D)
    return torch.cat([flat(dq), flat(dk), flat(dv)], 1)


def dhpre_step(df, hpre, w2, c, site_ff):
    """d hpre from d f AS STORED: (d f W2) * dropout * act'(hpre as saved) -> (value, magnitude sum, |d f W2| * dropout: what an
    absolute error of act' is multiplied with)."""
    df, w2 = _d(df), _d(w2)
    drop = row_drop(c.seed, site_ff, c.p, c.B * c.L, c.ff)
    mult = dact_fn(c.act, _d(hpre)) * drop
    return (df @ w2) * mult, (df.abs() @ w2.abs()) * mult.abs(), (df @ w2).abs() * drop


def layer_bwd(gy, sv, w, c, sites):
    """gy = gradient of the layer's output (fp64).  sv: x, qkv, a, x1, hpre, f, n1.mean, n1.rstd, n3.mean, n3.rstd as given to the kernel;
    sites = (self-attention probabilities, norm1, feed-forward, last norm).  Returns df, dhpre, da, dqkv, dx and the partial rows
    n3.ws / n1.ws [B, 2, 512]."""
    B, L, M = c.B, c.L, c.B * c.L
    sv = {k: _d(v) for k, v in sv.items()}
    r = {}
    ds3, r["df"], r["n3.ws"] = ln_bwd(gy, sv["f"], sv["x1"], row_drop(c.seed, sites[3], c.p, M, D), w["n3"][0], sv["n3.mean"], sv["n3.rstd"], B)
    r["dhpre"] = (r["df"] @ _d(w["w2"])) * dact_fn(c.act, sv["hpre"]) * row_drop(c.seed, sites[2], c.p, M, c.ff)
    g1 = ds3 + r["dhpre"] @ _d(w["w1"])
    ds1, r["da"], r["n1.ws"] = ln_bwd(g1, sv["a"], sv["x"], row_drop(c.seed, sites[1], c.p, M, D), w["n1"][0], sv["n1.mean"], sv["n1.rstd"], B)
    do = r["da"] @ _d(w["w_o"])
    r["dqkv"] = attention_bwd(do, sv["qkv"], B, L, c.causal, c.kpm, attn_drop(c.seed, sites[0], c.p, B, L, L))
    r["dx"] = ds1 + r["dqkv"] @ _d(w["w_in"])
    return r


def stack_bwd(dy, saved, layers, c, sites, final=None, y_last=None, nf_stats=None):
    """Top layer first: saved / layers / sites in FORWARD order.  final = gamma of the stack-final norm (y_last, nf_stats = (mean, rstd)
    given).  Returns (per-layer results in forward order, nf partial rows or None)."""
    gy, nf_ws = _d(dy), None
    if final is not None:
        gy, _, nf_ws = ln_bwd(gy, _d(y_last), None, 1.0, final, _d(nf_stats[0]), _d(nf_stats[1]), c.B)
    res = [None] * len(layers)
    for l in reversed(range(len(layers))):
        res[l] = layer_bwd(gy, saved[l], layers[l], c, sites[l])
        gy = res[l]["dx"]
    return res, nf_ws


# ---- stream order of the packed weights (include/vct_hip.h) ---------------------------------------------------------------------------------
def fwd_stream_table(ff, cross, first=0):
    """Blocks of ONE layer of vct_layer_ss_fwd's stream: (matrix, row0, col0, chunks, first chunk, transposed); each block = rows
    row0 .. row0+511 x columns col0 .. col0 + 64 * chunks - 1 of the [out, in] matrix."""
    t, at = [], first
    mats = [("w_in", 3), ("w_o", 1)] + ([("c_in", 3), ("c_o", 1)] if cross else [])
    for name, nb in mats:
        for i in range(nb):
            t.append((name, 512 * i, 0, 8, at, False)); at += 8
    nj = ff // 512
    t.append(("w1", 0, 0, 8, at, False)); at += 8
    for j in range(nj):
        if j + 1 < nj:
            t.append(("w1", 512 * (j + 1), 0, 8, at, False)); at += 8
        t.append(("w2", 0, 512 * j, 8, at, False)); at += 8
    return t


def bwd_stream_table(ff, first=0):
    """... of vct_layer_ss_bwd's stream: transposed segments (element (n, k) of the stream's matrix is w[row0 + k][col0 + n])."""
    t, at = [], first
    for j in range(ff // 512):
        t.append(("w2", 0, 512 * j, 8, at, True)); at += 8
        t.append(("w1", 512 * j, 0, 8, at, True)); at += 8
    t.append(("w_o", 0, 0, 8, at, True)); at += 8
    t.append(("w_in", 0, 0, 24, at, True)); at += 24
    return t


def pack_blocks(table, w):
    """The (view, chunks, first chunk, transposed) blocks ops.ss_pack takes, from a table and the layer's matrices."""
    return [(w[name][r0:, c0:], nch, at, tr) for name, r0, c0, nch, at, tr in table]


def packed_block(src, nch, tr):
    """Host restatement of one packed block: int16 [nch, 8 waves, 4 tiles, 2 k-steps, 64 lanes, 8] from the int16 matrix view `src`
    (numpy): lane l of fragment (wave, tile, k-step) of chunk c holds A[64 wave + 16 tile + (l & 15)][64 c + 32 k-step + 8 (l >> 4) + 0..7],
    A = src (plain) or src^T (transposed)."""
    A = src.T if tr else src
    lane = np.arange(64)
    out = np.empty((nch, 8, 4, 2, 64, 8), np.int16)
    for c_ in range(nch):
        for wv in range(8):
            for t in range(4):
                for s in range(2):
                    rows = wv * 64 + t * 16 + (lane & 15)
                    cols = c_ * 64 + s * 32 + (lane >> 4) * 8
                    out[c_, wv, t, s] = A[rows[:, None], cols[:, None] + np.arange(8)[None]]
    return out
