"""Tensor-level wrappers over the C ABI (include/vct_hip.h).  PyTorch supplies device memory and the
current HIP stream; every function here enqueues hand-written gfx950 kernels and nothing else."""
from typing import Optional, Tuple

import torch

from . import _lib as L

Drop = Optional[Tuple[torch.Tensor, int, float]]  # (seed tensor uint32[1] on device, site id, p)

# Live timing of tagged launches (bench.py roofline): see taps_enable / tap / tap_collect at the end of this file --
# HIP event pairs recorded by the C runtime on the launch stream, so they also fire inside replayed launch lists.


def _drop(d: Drop):
    if d is None or d[2] <= 0.0:
        return 0, 0, 0.0
    return d[0].data_ptr(), int(d[1]), float(d[2])


def _ld(t: torch.Tensor) -> int:
    assert t.dim() == 2 and t.stride(1) == 1, "row-major 2-D view required"
    return t.stride(0)


class GemmScratch:
    """Split-K scratch of ONE stream: fp32 partials + the zero-initialised tile counters that let the split-K
    reduction happen inside the producing kernel (include/vct_hip.h, tile_counters).  GEMMs that may run
    concurrently must use different GemmScratch objects."""
    COUNTERS_PER_SLOT = 16384

    def __init__(self, device, nbytes: int = 64 << 20):
        self.ws = torch.empty(nbytes // 4, dtype=torch.float32, device=device)
        self.counters = torch.zeros(L.GEMM_GROUP_MAX * self.COUNTERS_PER_SLOT, dtype=torch.int32, device=device)


def _gemm_desc(a, b, out, ta, tb, bias, act, preact, addend, dact_src, dropout, bias_grad, workspace, split_k,
               n_valid, k_valid, m_valid, adam=None):
    d = L.GemmDesc()
    if adam is not None:      # L.GemmAdam: optimizer epilogue of the weight-gradient form (the caller keeps it alive through the call)
        d.adam = L.C.pointer(adam)
    d.dtype, d.out_dtype = L.dtype_code(a.dtype), L.dtype_code(out.dtype)
    assert b.dtype == a.dtype
    d.ta, d.tb = int(ta), int(tb)
    M = a.shape[1] if ta else a.shape[0]
    K = a.shape[0] if ta else a.shape[1]
    N = b.shape[0] if tb else b.shape[1]
    Kb = b.shape[1] if tb else b.shape[0]
    if k_valid is not None:
        K = k_valid
    else:
        assert K == Kb, (a.shape, b.shape, ta, tb)
    if n_valid is not None:
        N = n_valid
    if m_valid is not None:
        M = m_valid
    d.M, d.N, d.K = M, N, K
    d.act = L.ACT[act]
    d.A, d.lda, d.B, d.ldb, d.C, d.ldc = a.data_ptr(), _ld(a), b.data_ptr(), _ld(b), out.data_ptr(), _ld(out)
    d.bias = L.ptr(bias)
    if preact is not None:
        d.preact, d.ld_preact = preact.data_ptr(), _ld(preact)
    if addend is not None:
        d.addend, d.ld_addend = addend.data_ptr(), _ld(addend)
    if dact_src is not None:
        d.dact_src, d.ld_dact = dact_src.data_ptr(), _ld(dact_src)
    d.seed, d.site, d.p_drop = _drop(dropout)
    d.bias_grad = L.ptr(bias_grad)
    if isinstance(workspace, GemmScratch):
        d.workspace, d.workspace_bytes = workspace.ws.data_ptr(), workspace.ws.numel() * 4
        d.tile_counters, d.n_tile_counters = workspace.counters.data_ptr(), GemmScratch.COUNTERS_PER_SLOT
    elif workspace is not None:
        d.workspace, d.workspace_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
    d.split_k = split_k
    return d


def gemm(a: torch.Tensor, b: torch.Tensor, out: torch.Tensor, *, ta: bool = False, tb: bool = True,
         bias: Optional[torch.Tensor] = None, act: Optional[str] = None, preact: Optional[torch.Tensor] = None,
         addend: Optional[torch.Tensor] = None, dact_src: Optional[torch.Tensor] = None, dropout: Drop = None,
         bias_grad: Optional[torch.Tensor] = None, workspace=None, split_k: int = 0,
         n_valid: Optional[int] = None, k_valid: Optional[int] = None, m_valid: Optional[int] = None,
         tag: Optional[str] = None, tile: int = 0, adam=None) -> torch.Tensor:
    """out[M,N] = epilogue(op(a) @ op(b)).  ta=False: a is [M,K]; ta=True: a is [K,M].
    tb=True: b is [N,K] (nn.Linear weight); tb=False: b is [K,N].  n_valid / k_valid override the
    logical N / K when a buffer is wider than its valid extent (zero-padded vocabulary columns).
    workspace: a fp32 tensor (two-pass split-K) or a GemmScratch (single-pass split-K).
    adam: L.GemmAdam (weight-gradient form only) -- torch.optim.Adam's step on the matrix runs in the epilogue (include/vct_hip.h)."""
    lib = L.load()
    d = _gemm_desc(a, b, out, ta, tb, bias, act, preact, addend, dact_src, dropout, bias_grad, workspace, split_k,
                   n_valid, k_valid, m_valid, adam)
    d.reserved = tile       # kernel selection override (include/vct_hip.h, vct_gemm_desc.reserved): tests and A/B probes
    timed = _taps_on and tag in TAPS and (_taps_only is None or tag in _taps_only)
    if timed:
        tap(tag, 0)
    L.check(lib.vct_gemm(d, L.stream_ptr()), "vct_gemm")
    if timed:
        tap(tag, 1)
    return out


def gemm_grouped(items, scratch: GemmScratch, split_k: int = 0, tile: int = 0):
    """One launch for up to 8 weight-gradient GEMMs: items = [(dy [rows,M], x [rows,N], dW [M,N] fp32, db [M] fp32 or None[, L.GemmAdam or None])]
    -> dW = dy^T x, db = column sums of dy (include/vct_hip.h, vct_gemm_grouped); with a GemmAdam the optimizer steps the matrix in
    the epilogue."""
    lib = L.load()
    n = len(items)
    if not 1 <= n <= L.GEMM_GROUP_MAX:
        raise ValueError(f"gemm_grouped: 1..{L.GEMM_GROUP_MAX} problems per launch, got {n}")
    arr = (L.GemmDesc * n)()
    for i, it in enumerate(items):
        dy, x, dw, db = it[:4]
        d = _gemm_desc(dy, x, dw, True, False, None, None, None, None, None, None, db, None, split_k, None, None, None,
                       it[4] if len(it) > 4 else None)
        C_ = L.C
        C_.memmove(C_.byref(arr[i]), C_.byref(d), C_.sizeof(L.GemmDesc))
    arr[0].reserved = tile
    off = 0
    for i in range(n):
        need = int(lib.vct_gemm_grouped_workspace_bytes(arr, n, i))
        need = (need + 255) // 256 * 256
        arr[i].workspace, arr[i].workspace_bytes = scratch.ws.data_ptr() + off, need
        arr[i].tile_counters = scratch.counters.data_ptr() + 4 * i * GemmScratch.COUNTERS_PER_SLOT
        arr[i].n_tile_counters = GemmScratch.COUNTERS_PER_SLOT
        off += need
    if off > scratch.ws.numel() * 4:
        raise ValueError(f"gemm_grouped: scratch too small ({off} > {scratch.ws.numel() * 4} bytes)")
    L.check(lib.vct_gemm_grouped(arr, n, L.stream_ptr()), "vct_gemm_grouped")


_ROUTE_KERNELS = {0: None, 1: "general_bf16", 2: "general_f32", 3: "skinny", 4: "g256", 5: "g256_g32", 6: "layer_pt", 7: "grouped"}


def gemm_last_route() -> dict:
    """The route this thread's last gemm / gemm_grouped took (include/vct_hip.h, vct_gemm_last_route): kernel id and name, tile,
    operand stages, variant id, split, where the split was reduced; for a grouped launch also each problem's split."""
    lib = L.load()
    buf = (L.i32 * L.GEMM_ROUTE_INTS)()
    L.check(lib.vct_gemm_last_route(buf, L.GEMM_ROUTE_INTS), "vct_gemm_last_route")
    r = list(buf)
    return {"kernel": r[0], "name": _ROUTE_KERNELS.get(r[0]), "bm": r[1], "bn": r[2], "nbuf": r[3], "variant": r[4], "split": r[5],
            "in_kernel_reduce": bool(r[6]), "reduce_launch": bool(r[7]), "group_splits": r[9:9 + r[8]]}


def gemm_workspace_bytes(M: int, N: int, K: int, dtype: torch.dtype) -> int:
    """Upper bound of the split-K workspace the weight-gradient GEMM [M,N] (reduction K) may use."""
    lib = L.load()
    d = L.GemmDesc()
    d.dtype, d.out_dtype, d.ta, d.tb, d.M, d.N, d.K = L.dtype_code(dtype), L.F32, 1, 0, M, N, K
    return int(lib.vct_gemm_workspace_bytes(d))


def _attn_desc(dtype, B, H, Lq, Lk, hd, causal, q, k, v, key_pad, dropout):
    d = L.AttnDesc()
    d.dtype, d.B, d.H, d.Lq, d.Lk, d.hd, d.causal = L.dtype_code(dtype), B, H, Lq, Lk, hd, int(causal)
    d.q, d.ldq, d.k, d.ldk, d.v, d.ldv = q.data_ptr(), _ld(q), k.data_ptr(), _ld(k), v.data_ptr(), _ld(v)
    # key_pad: uint8/bool [B, Lk] | (mask [B, Lk - shift], shift) = first `shift` keys never padded | ("ids", ids [B, >=Lk] int64, pad_id)
    if isinstance(key_pad, tuple) and key_pad[0] == "ids":
        _tag, ids, pad_id = key_pad
        assert ids.dtype == torch.int64 and ids.stride(1) == 1 and ids.shape[1] >= Lk
        d.key_ids, d.key_ids_bs, d.pad_id = ids.data_ptr(), ids.stride(0), int(pad_id)
    elif isinstance(key_pad, tuple):
        m, shift = key_pad
        assert m.is_contiguous() and m.element_size() == 1 and tuple(m.shape) == (B, Lk - shift)
        d.key_pad, d.key_pad_shift = m.data_ptr(), int(shift)
    else:
        d.key_pad = L.ptr(key_pad)
    d.seed, d.site, d.p_drop = _drop(dropout)
    return d


def attn_fwd(q, k, v, o, B, H, Lq, Lk, causal=False, key_pad=None, dropout: Drop = None, kv_batch_stride: int = 0):
    """q:[B*Lq, >=H*hd] views (any row stride), k,v:[B*Lk, ..]; o:[B*Lq, H*hd].  key_pad: uint8 [B,Lk].
    kv_batch_stride (elements): K/V live in a cache [B, Lmax, ...] and only the first Lk rows of each batch are read."""
    hd = o.shape[1] // H
    d = _attn_desc(q.dtype, B, H, Lq, Lk, hd, causal, q, k, v, key_pad, dropout)
    d.o, d.ldo = o.data_ptr(), _ld(o)
    d.k_bs = d.v_bs = kv_batch_stride
    L.check(L.load().vct_attn_fwd(d, L.stream_ptr()), "vct_attn_fwd")
    return o


def attn_weights(q, k, w, B, H, Lq, Lk, causal=False, key_pad=None, kv_batch_stride: int = 0):
    """w fp32 [B, Lq, Lk] view (last dimension contiguous, any row / batch stride) = mean over the H heads of
    softmax(q k^T / sqrt(hd) + mask): nn.MultiheadAttention's averaged attention weights (include/vct_hip.h, vct_attn_weights).
    q: [B*Lq, >=H*hd] view, k: [B*Lk, ..] view, key_pad / kv_batch_stride as attn_fwd."""
    assert w.dtype == torch.float32 and tuple(w.shape) == (B, Lq, Lk) and w.stride(2) == 1
    hd = q.shape[1] // H
    src = _attn_desc(q.dtype, B, H, Lq, Lk, hd, causal, q, k, k, key_pad, None)
    d = L.AttnWeightsDesc()
    for f in ("dtype", "B", "H", "Lq", "Lk", "hd", "causal", "key_pad_shift", "q", "ldq", "k", "ldk", "key_pad",
              "key_ids", "key_ids_bs", "pad_id"):
        setattr(d, f, getattr(src, f))
    d.w, d.ldw, d.w_bs = w.data_ptr(), (w.stride(1) if Lq > 1 else Lk), w.stride(0)
    d.k_bs = kv_batch_stride
    L.check(L.load().vct_attn_weights(d, L.stream_ptr()), "vct_attn_weights")
    return w


# ---- sample-stationary layer forward (csrc/vct_layer_ss.hip) ---------------------------------------------------------------------
_ss_ok = {}
SS_CHUNK = 32768          # bf16 elements per 64-KiB chunk of a packed weight stream


def layer_ss_supported(dtype, d: int, H: int, ff: int, L_: int, Lm: int) -> bool:
    if dtype != torch.bfloat16:
        return False
    key = (d, H, ff, L_, Lm)
    r = _ss_ok.get(key)
    if r is None:
        r = _ss_ok[key] = bool(L.load().vct_layer_ss_supported(L.BF16, d, H, ff, L_, Lm))
    return r


def layer_ss_stream_chunks(ff: int, cross: bool) -> int:
    return int(L.load().vct_layer_ss_stream_chunks(int(ff), int(cross)))


def ss_pack(blocks, dst: torch.Tensor):
    """blocks: [(w2d bf16 view whose rows 0..511 x columns 0..64*nchunks-1 form the block, nchunks, dst_chunk)] -> the packed stream
    `dst` (bf16, stream order: include/vct_hip.h, vct_ss_pack).  One launch per 48 blocks."""
    n = len(blocks)
    segs = (L.SsPackSeg * n)()
    for i, blk in enumerate(blocks):
        w, nch, dc = blk[:3]
        tr = bool(blk[3]) if len(blk) > 3 else False        # transposed block: element (n, k) of the stream's matrix is w[k][n]
        if tr:
            assert w.dtype == torch.bfloat16 and w.stride(1) == 1 and w.shape[1] >= 512 and w.shape[0] >= 64 * nch
        else:
            assert w.dtype == torch.bfloat16 and w.stride(1) == 1 and w.shape[0] >= 512 and w.shape[1] >= 64 * nch
        segs[i].w, segs[i].ldw, segs[i].nchunks, segs[i].dst_chunk = w.data_ptr(), w.stride(0), int(nch), int(dc)
        segs[i].transposed = int(tr)
    L.check(L.load().vct_ss_pack(segs, n, dst.data_ptr(), L.stream_ptr()), "vct_ss_pack")
    return dst


def layer_ss_bwd_stream_chunks(ff: int) -> int:
    return int(L.load().vct_layer_ss_bwd_stream_chunks(int(ff)))


def layer_ss_bwd_desc(*, B, Lr, wpk, nchunks, ff, act, H, x, qkv, a, x1, hpre, f, n1, n3, outs, sites, nf=None, y_last=None, dy=None, dx=None,
                      causal=False, key_pad=None, seed=None, p_drop=0.0):
    """Descriptor of ONE layer of a sample-stationary backward launch (include/vct_hip.h, vct_layer_ss_bwd_desc).  nX = (gamma, mean,
    rstd, ws[B, 2, 512] fp32); outs = (df, dhpre, da, dqkv); sites = (self-attention probabilities, norm1, feed-forward, last norm)."""
    q = L.LayerSsBwdDesc()
    q.dtype, q.B, q.L, q.d, q.H, q.ff, q.act = L.BF16, int(B), int(Lr), x.shape[1], int(H), int(ff), L.ACT[act]
    q.last, q.causal = int(nf is not None), int(causal)
    q.wpk, q.nchunks = wpk.data_ptr(), int(nchunks)
    q.dy, q.dx, q.y_last = L.ptr(dy), L.ptr(dx), L.ptr(y_last)
    q.x, q.qkv, q.a, q.x1, q.hpre, q.f = (t.data_ptr() for t in (x, qkv, a, x1, hpre, f))

    def norm(dst, t):
        dst.gamma, dst.mean, dst.rstd, dst.ws = (z.data_ptr() for z in t)
    norm(q.n1, n1)
    norm(q.n3, n3)
    if nf is not None:
        norm(q.nf, nf)
    q.df, q.dhpre, q.da, q.dqkv = (t.data_ptr() for t in outs)
    q.key_pad_shift = 0
    if isinstance(key_pad, tuple) and key_pad[0] == "ids":
        _tag, ids, pad_id = key_pad
        q.key_ids, q.key_ids_bs, q.pad_id = ids.data_ptr(), ids.stride(0), int(pad_id)
    elif isinstance(key_pad, tuple):
        m, shift = key_pad
        q.key_pad, q.key_pad_shift = m.data_ptr(), int(shift)
    elif key_pad is not None:
        q.key_pad = key_pad.data_ptr()
    q.seed, q.p_drop = L.ptr(seed), float(p_drop)
    q.site_sa, q.site_n1, q.site_ff, q.site_n3 = (int(z) for z in sites)
    return q


def layer_ss_bwd(descs):
    """One launch: the activation-gradient chain of a self-attention + feed-forward stack, descs[0] = the TOP layer."""
    n = len(descs)
    arr = (L.LayerSsBwdDesc * n)(*descs)
    L.check(L.load().vct_layer_ss_bwd(arr, n, L.stream_ptr()), "vct_layer_ss_bwd")


def layer_ss_desc(*, B, Lr, x, wpk, nchunks, ff, act, H, bias, sa, n1, ffn, n3, cross=None, n2=None, nf=None, mem=None, Lm=0,
                  causal=False, key_pad=None, seed=None, p_drop=0.0, sites=(0, 0, 0, 0, 0, 0), frontend=None, embed=None):
    """Descriptor of ONE layer of a sample-stationary stack launch (include/vct_hip.h, vct_layer_ss_desc).  bias = dict(qkv, o,
    [cq, ckv, co], l1, l2) fp32 vectors; sa = (qkv, o, a); cross = (q, kv, o, a); ffn = (hpre, h, f); nX = (gamma, beta, y, mean, rstd);
    sites = dropout sites (self-attention probabilities, norm1, cross-attention probabilities, norm2, feed-forward, norm3)."""
    q = L.LayerSsDesc()
    q.dtype, q.B, q.L, q.Lm, q.d, q.H, q.ff, q.act = L.BF16, int(B), int(Lr), int(Lm), x.shape[1], int(H), int(ff), L.ACT[act]
    q.last, q.causal = int(nf is not None), int(causal)
    q.wpk, q.nchunks, q.x, q.mem = wpk.data_ptr(), int(nchunks), x.data_ptr(), L.ptr(mem)

    def norm(dst, t):
        dst.gamma, dst.beta, dst.y, dst.mean, dst.rstd = (z.data_ptr() for z in t)
    q.b_qkv, q.b_o = bias["qkv"].data_ptr(), bias["o"].data_ptr()
    q.qkv, q.o, q.a = (t.data_ptr() for t in sa)
    norm(q.n1, n1)
    if cross is not None:
        q.b_cq, q.b_ckv, q.b_co = bias["cq"].data_ptr(), bias["ckv"].data_ptr(), bias["co"].data_ptr()
        q.cq, q.ckv, q.co, q.ca = (t.data_ptr() for t in cross)
        norm(q.n2, n2)
    q.b1, q.b2 = bias["l1"].data_ptr(), bias["l2"].data_ptr()
    q.hpre, q.h, q.f = (t.data_ptr() for t in ffn)
    norm(q.n3, n3)
    if nf is not None:
        norm(q.nf, nf)
    if isinstance(key_pad, tuple) and key_pad[0] == "ids":
        _tag, ids, pad_id = key_pad
        assert ids.dtype == torch.int64 and ids.stride(1) == 1 and ids.shape[1] >= Lr
        q.key_ids, q.key_ids_bs, q.pad_id = ids.data_ptr(), ids.stride(0), int(pad_id)
    elif isinstance(key_pad, tuple):
        m, shift = key_pad
        assert m.is_contiguous() and m.element_size() == 1 and tuple(m.shape) == (B, Lr - shift)
        q.key_pad, q.key_pad_shift = m.data_ptr(), int(shift)
    elif key_pad is not None:
        q.key_pad = key_pad.data_ptr()
    if seed is not None and p_drop > 0.0:
        q.seed, q.p_drop = seed.data_ptr(), float(p_drop)
    q.site_sa, q.site_n1, q.site_ca, q.site_n2, q.site_ff, q.site_n3 = (int(s) for s in sites)
    if frontend is not None:       # (feats [B*T, 512] fp32 / bf16, x_in bf16 copy or None, unify bias, PE' rows [T+1, 512]): x is built and stored
        feats, x_in, b_u, pe_rows = frontend
        q.pro, q.feats_dtype, q.feats, q.x_in = 1, L.dtype_code(feats.dtype), feats.data_ptr(), L.ptr(x_in)
        q.b_unify, q.pe_rows = b_u.data_ptr(), pe_rows.data_ptr()
    if embed is not None:          # (ids [B, >= L] int64, fp32 table, fp32 positional rows, dropout site): x is built and stored
        ids, table, pos, site = embed
        assert ids.dtype == torch.int64 and ids.stride(1) == 1 and ids.shape[1] >= Lr
        q.pro, q.emb_ids, q.emb_ids_bs, q.emb_table, q.emb_pos, q.site_emb = 2, ids.data_ptr(), ids.stride(0), table.data_ptr(), pos.data_ptr(), int(site)
    return q


def layer_ss_fwd(descs):
    """A whole stack (list of layer_ss_desc results, first layer first) in ceil(n / 4) launches (vct_layer_ss_fwd)."""
    arr = (L.LayerSsDesc * len(descs))(*descs)
    L.check(L.load().vct_layer_ss_fwd(arr, len(descs), L.stream_ptr()), "vct_layer_ss_fwd")


def attn_bwd(q, k, v, d_o, dq, dk, dv, B, H, Lq, Lk, causal=False, key_pad=None, dropout: Drop = None):
    hd = d_o.shape[1] // H
    d = _attn_desc(q.dtype, B, H, Lq, Lk, hd, causal, q, k, v, key_pad, dropout)
    d.d_o, d.ld_do = d_o.data_ptr(), _ld(d_o)
    d.dq, d.ld_dq, d.dk, d.ld_dk, d.dv, d.ld_dv = dq.data_ptr(), _ld(dq), dk.data_ptr(), _ld(dk), dv.data_ptr(), _ld(dv)
    L.check(L.load().vct_attn_bwd(d, L.stream_ptr()), "vct_attn_bwd")


def add_ln_fwd(x, res, gamma, beta, y, mean, rstd, dropout: Drop = None):
    M, dm = x.shape
    s, site, p = _drop(dropout)
    L.check(L.load().vct_add_ln_fwd(L.dtype_code(x.dtype), M, dm, x.data_ptr(), L.ptr(res), gamma.data_ptr(),
                                    beta.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), s, site, p,
                                    L.stream_ptr()), "vct_add_ln_fwd")
    return y


def add_ln_ln_fwd(x, res, gamma, beta, y, mean, rstd, gamma2, beta2, y2, mean2, rstd2, dropout: Drop = None):
    """y = LayerNorm(res + dropout(x)); y2 = LayerNorm2(y) -- a layer's last norm and the stack-final norm in one launch."""
    M, dm = x.shape
    s, site, p = _drop(dropout)
    L.check(L.load().vct_add_ln_ln_fwd(L.dtype_code(x.dtype), M, dm, x.data_ptr(), L.ptr(res), gamma.data_ptr(), beta.data_ptr(),
                                       y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma2.data_ptr(), beta2.data_ptr(),
                                       y2.data_ptr(), mean2.data_ptr(), rstd2.data_ptr(), s, site, p, L.stream_ptr()),
            "vct_add_ln_ln_fwd")
    return y2


def ln_ws_rows(M: int) -> int:
    return int(L.load().vct_ln_ws_rows(M))


def add_ln_bwd(dy, x, res, gamma, mean, rstd, ds, dxo, dgamma, dbeta, param_ws, dropout: Drop = None):
    M, dm = x.shape
    s, site, p = _drop(dropout)
    L.check(L.load().vct_add_ln_bwd(L.dtype_code(x.dtype), M, dm, dy.data_ptr(), x.data_ptr(), L.ptr(res),
                                    gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(), ds.data_ptr(), L.ptr(dxo),
                                    L.ptr(dgamma), L.ptr(dbeta), param_ws.data_ptr(), s, site, p,
                                    L.stream_ptr()), "vct_add_ln_bwd")


def add_ln_ln_bwd(dy2, y, gamma2, mean2, rstd2, param_ws2, x, res, gamma, mean, rstd, ds, dxo, param_ws, dropout: Drop = None):
    """Backward of add_ln_ln_fwd in one launch (include/vct_hip.h, vct_add_ln_ln_bwd): the stack-final norm, then the last layer's norm."""
    M, dm = x.shape
    s, site, p = _drop(dropout)
    L.check(L.load().vct_add_ln_ln_bwd(L.dtype_code(x.dtype), M, dm, dy2.data_ptr(), y.data_ptr(), gamma2.data_ptr(), mean2.data_ptr(),
                                       rstd2.data_ptr(), param_ws2.data_ptr(), x.data_ptr(), L.ptr(res), gamma.data_ptr(), mean.data_ptr(),
                                       rstd.data_ptr(), ds.data_ptr(), L.ptr(dxo), param_ws.data_ptr(), s, site, p, L.stream_ptr()),
            "vct_add_ln_ln_bwd")


def ln_param_finalize_batched(table, n_entries, d):
    """table: int64 device tensor [n_entries, 4] = (param_ws ptr, dgamma ptr, dbeta ptr, ws rows)."""
    L.check(L.load().vct_ln_param_finalize_batched(table.data_ptr(), n_entries, d, L.stream_ptr()), "vct_ln_param_finalize_batched")


def enc_frontend_fwd(u, pe_rows, z, B, T):
    L.check(L.load().vct_enc_frontend_fwd(L.dtype_code(u.dtype), B, T, u.shape[1], u.data_ptr(), pe_rows.data_ptr(),
                                          z.data_ptr(), L.stream_ptr()), "vct_enc_frontend_fwd")
    return z


def enc_frontend_bwd(dz, du, B, T):
    L.check(L.load().vct_enc_frontend_bwd(L.dtype_code(dz.dtype), B, T, dz.shape[1], dz.data_ptr(), du.data_ptr(),
                                          L.stream_ptr()), "vct_enc_frontend_bwd")
    return du


def _mm_desc(dtype, B, d, Ts, labels, n_labels):
    if not 2 <= len(Ts) <= L.MM_MAX_MODAL:
        raise ValueError(f"multi-modal front end: 2..{L.MM_MAX_MODAL} modalities, got {len(Ts)}")
    if labels.dtype != torch.int32 or labels.numel() != sum(t + 1 for t in Ts):
        raise ValueError("multi-modal front end: labels must be int32 [sum(T_i + 1)]")
    desc = L.MmFrontendDesc()
    desc.dtype, desc.n, desc.B, desc.d, desc.n_labels = L.dtype_code(dtype), len(Ts), B, d, n_labels
    for i, t in enumerate(Ts):
        desc.T[i] = int(t)
    desc.labels = labels.data_ptr()
    return desc


def mm_frontend_fwd(us, masks, temp, modal_w, labels, x0, key_pad, B, Ts):
    """Multi-modal front end (include/vct_hip.h, vct_mm_frontend_fwd): us[i] [B*T_i, d] unify outputs, masks[i] uint8 [B, T_i] or
    None, temp fp32 [S, d], modal_w fp32 [n_labels, d], labels int32 [S] -> x0 [B*S, d], key_pad uint8 [B, S] (or None)."""
    d = x0.shape[-1]
    desc = _mm_desc(x0.dtype, B, d, Ts, labels, modal_w.shape[0])
    for i, u in enumerate(us):
        desc.u[i] = u.data_ptr()
        desc.mask[i] = L.ptr(masks[i]) if masks is not None else 0
    desc.temp, desc.modal_w, desc.x0, desc.key_pad = temp.data_ptr(), modal_w.data_ptr(), x0.data_ptr(), L.ptr(key_pad)
    L.check(L.load().vct_mm_frontend_fwd(L.C.byref(desc), L.stream_ptr()), "vct_mm_frontend_fwd")
    return x0


def mm_frontend_bwd(dx, dus, d_modal, labels, B, Ts):
    """Backward of mm_frontend_fwd: dus[i] [B*T_i, d] <- dx [B*S, d]; d_modal fp32 [n_labels, d] is WRITTEN."""
    desc = _mm_desc(dx.dtype, B, dx.shape[-1], Ts, labels, d_modal.shape[0])
    for i, du in enumerate(dus):
        desc.du[i] = du.data_ptr()
    desc.dx, desc.d_modal = dx.data_ptr(), d_modal.data_ptr()
    L.check(L.load().vct_mm_frontend_bwd(L.C.byref(desc), L.stream_ptr()), "vct_mm_frontend_bwd")
    return dus


def _fx_desc(dtype, B, d, Ts, agg, temp, emb_w, tidx, modal_w, labels, norm):
    """The part of vct_enc_frontend_ex_desc both directions share.  agg 'avg' | 'max'; temporal source: temp fp32 [S, d] (fixed table)
    or emb_w fp32 [rows, d] with tidx int32 [S] (learned); modal_w / labels: None with one stream; norm: None or the dict of
    enc_frontend_ex_fwd."""
    n, S = len(Ts), sum(t + 1 for t in Ts)
    if not 1 <= n <= L.MM_MAX_MODAL:
        raise ValueError(f"encoder front end: 1..{L.MM_MAX_MODAL} feature streams, got {n}")
    if (temp is None) == (tidx is None):
        raise ValueError("encoder front end: exactly one temporal source (the fixed table, or the embedding weight with its row indices)")
    if tidx is not None and (tidx.dtype != torch.int32 or tidx.numel() != S):
        raise ValueError("encoder front end: tidx must be int32 [sum(T_i + 1)]")
    if n >= 2 and (labels is None or labels.dtype != torch.int32 or labels.numel() != S):
        raise ValueError("encoder front end: labels must be int32 [sum(T_i + 1)]")
    desc = L.EncFrontendExDesc()
    desc.dtype, desc.n, desc.B, desc.d, desc.agg = L.dtype_code(dtype), n, B, d, L.AGG[agg]
    for i, t in enumerate(Ts):
        desc.T[i] = int(t)
    if tidx is not None:
        desc.temporal, desc.tidx, desc.emb_w, desc.emb_rows = L.TEMPORAL["embedding"], tidx.data_ptr(), L.ptr(emb_w), emb_w.shape[0]
    else:
        desc.temporal, desc.temp = L.TEMPORAL["encoding"], temp.data_ptr()
    if n >= 2:
        desc.labels, desc.modal_w, desc.n_labels = labels.data_ptr(), L.ptr(modal_w), modal_w.shape[0]
    if norm is not None:
        s, site, p = _drop(norm.get("dropout"))
        desc.norm, desc.gamma, desc.beta, desc.mean, desc.rstd = 1, norm["gamma"].data_ptr(), L.ptr(norm.get("beta")), \
            norm["mean"].data_ptr(), norm["rstd"].data_ptr()
        desc.seed, desc.site, desc.p_drop = s, site, p
    return desc


def enc_frontend_ex_fwd(us, masks, x0, key_pad, B, Ts, *, agg="avg", temp=None, emb_w=None, tidx=None, modal_w=None, labels=None,
                        norm=None):
    """Encoder front end with every `mme` option (include/vct_hip.h, vct_enc_frontend_ex_fwd), n >= 1 streams: us[i] [B*T_i, d],
    masks[i] uint8 [B, T_i] or None -> x0 [B*S, d], key_pad uint8 [B, S] (or None).  norm: None, or dict(gamma, beta fp32 [d],
    mean, rstd fp32 [B*S] (written), dropout = (seed, site, p) or None): x0 = dropout(LayerNorm(pre))."""
    desc = _fx_desc(x0.dtype, B, x0.shape[-1], Ts, agg, temp, emb_w, tidx, modal_w, labels, norm)
    for i, u in enumerate(us):
        desc.u[i] = u.data_ptr()
        desc.mask[i] = L.ptr(masks[i]) if masks is not None else 0
    desc.x0, desc.key_pad = x0.data_ptr(), L.ptr(key_pad)
    L.check(L.load().vct_enc_frontend_ex_fwd(L.C.byref(desc), L.stream_ptr()), "vct_enc_frontend_ex_fwd")
    return x0


def enc_frontend_ex_bwd(dx, dus, B, Ts, *, agg="avg", us=None, temp=None, emb_w=None, tidx=None, modal_w=None, labels=None,
                        d_modal=None, d_emb=None, norm=None, dpre=None, param_ws=None):
    """Backward of enc_frontend_ex_fwd: dus[i] [B*T_i, d] <- dx [B*S, d]; d_modal fp32 [n_labels, d] (n >= 2) and d_emb fp32
    [rows, d] (learned temporal) are WRITTEN.  us: the forward's unify outputs (agg 'max' or norm).  norm: the forward's dict
    (gamma, mean, rstd, dropout); then dpre fp32 [B*S, d] and param_ws fp32 [B*n*2*d] receive the pre-norm gradient and the
    norm-parameter partials (ln_param_finalize_batched with B*n rows sums them)."""
    desc = _fx_desc(dx.dtype, B, dx.shape[-1], Ts, agg, temp, emb_w, tidx, modal_w, labels, norm)
    for i, du in enumerate(dus):
        desc.du[i] = du.data_ptr()
        desc.u[i] = us[i].data_ptr() if us is not None else 0
    desc.dx, desc.d_modal, desc.d_emb, desc.dpre, desc.param_ws = dx.data_ptr(), L.ptr(d_modal), L.ptr(d_emb), L.ptr(dpre), L.ptr(param_ws)
    L.check(L.load().vct_enc_frontend_ex_bwd(L.C.byref(desc), L.stream_ptr()), "vct_enc_frontend_ex_bwd")
    return dus


def _hmm_desc(t, B, S, take):
    if t.dim() != 2 or t.shape[0] != B * S:
        raise ValueError(f"hierarchical encoder mix: rows [B*S, d] = [{B * S}, d] expected, got {tuple(t.shape)}")
    if take is not None and (take.dtype != torch.uint8 or take.numel() != S or not take.is_contiguous()):
        raise ValueError("hierarchical encoder mix: take must be contiguous uint8 [S]")
    desc = L.HmmMixDesc()
    desc.dtype, desc.B, desc.S, desc.d, desc.take = L.dtype_code(t.dtype), B, S, t.shape[1], L.ptr(take)
    return desc


def hmm_mix_fwd(y, x0, take, x, B, S):
    """Input of a layer of the hierarchical encoder (include/vct_hip.h, vct_hmm_mix_fwd): x[b, s] = y[b, s] (the previous layer's
    output) where take[s], else x0[b, s] (the stack input); y / x0 / x [B*S, d], take uint8 [S]."""
    desc = _hmm_desc(x, B, S, take)
    desc.y, desc.x0, desc.x = y.data_ptr(), x0.data_ptr(), x.data_ptr()
    L.check(L.load().vct_hmm_mix_fwd(L.C.byref(desc), L.stream_ptr()), "vct_hmm_mix_fwd")
    return x


def hmm_mix_bwd(dx, take, acc, B, S, *, dy=None, dx0=None, init: bool = False):
    """Backward of hmm_mix_fwd from the gradient dx [B*S, d] of a layer's input, acc fp32 [B*S, d]: dy <- dx on the continuing rows
    and 0 on the others, acc <- the restarting rows (init: written, 0 elsewhere; else added to).  At layer 0 (take = None):
    dx0 <- acc + dx, nothing else is written.  Returns dy (or dx0)."""
    if acc.dtype != torch.float32 or tuple(acc.shape) != tuple(dx.shape):
        raise ValueError("hierarchical encoder mix: acc must be fp32 with the shape of dx")
    if (dy is None) == (dx0 is None):
        raise ValueError("hierarchical encoder mix: exactly one of dy (layers above 0) and dx0 (layer 0)")
    desc = _hmm_desc(dx, B, S, take if dx0 is None else None)
    desc.dx, desc.dy, desc.acc, desc.dx0, desc.init = dx.data_ptr(), L.ptr(dy), acc.data_ptr(), L.ptr(dx0), int(bool(init))
    L.check(L.load().vct_hmm_mix_bwd(L.C.byref(desc), L.stream_ptr()), "vct_hmm_mix_bwd")
    return dy if dx0 is None else dx0


def embed_fwd(ids, S, table, pos, x, dropout: Drop = None):
    """ids: int64 [B, S_total] (row stride = ids.stride(0)); uses the first S columns of each row."""
    B = ids.shape[0]
    s, site, p = _drop(dropout)
    L.check(L.load().vct_embed_fwd(L.dtype_code(x.dtype), B, S, x.shape[1], ids.data_ptr(), ids.stride(0),
                                   table.data_ptr(), pos.data_ptr(), x.data_ptr(), s, site, p, L.stream_ptr()),
            "vct_embed_fwd")
    return x


def preln_fwd(x, gamma, beta, y):
    """y = LayerNorm(x): x the fp32 residual stream [M, d] of a pre-LN stack, y [M, d] fp32 or bf16 (include/vct_hip.h, vct_preln_fwd)."""
    M, dm = x.shape
    assert x.dtype == torch.float32 and x.is_contiguous() and y.is_contiguous() and tuple(y.shape) == (M, dm)
    assert gamma.dtype == beta.dtype == torch.float32 and gamma.numel() == beta.numel() == dm
    L.check(L.load().vct_preln_fwd(L.dtype_code(y.dtype), M, dm, x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(),
                                   L.stream_ptr()), "vct_preln_fwd")
    return y


def text_pool(ids, x, S, gamma, beta, y, eot, err):
    """y[b] = LayerNorm(x[b * S + e_b]), e_b = first index of the maximum of ids[b] (all columns of ids are scanned), eot[b] = e_b.
    ids int64 [B, >= S]; x fp32 [B * S, d]; y [B, d] fp32 or bf16; eot int32 [B]; err int32 [1], raised when an e_b lies behind S
    (include/vct_hip.h, vct_text_pool)."""
    B, dm = y.shape
    assert ids.dtype == torch.int64 and ids.dim() == 2 and ids.shape[0] == B and ids.stride(1) == 1 and ids.shape[1] >= S
    assert x.dtype == torch.float32 and x.is_contiguous() and tuple(x.shape) == (B * S, dm) and y.is_contiguous()
    assert gamma.dtype == beta.dtype == torch.float32 and gamma.numel() == beta.numel() == dm
    assert eot.dtype == torch.int32 and eot.numel() >= B and err.dtype == torch.int32 and err.numel() >= 1
    L.check(L.load().vct_text_pool(L.dtype_code(y.dtype), B, S, ids.shape[1], dm, ids.data_ptr(), ids.stride(0), x.data_ptr(),
                                   gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), eot.data_ptr(), err.data_ptr(), L.stream_ptr()),
            "vct_text_pool")
    return y


_embed_ws = {}
_embed_ws_retired = []
_embed_live = {}


def embed_live_table(dtable, create: bool = False):
    """The per-row "live" table of a gradient table (uint8 [V], owned with its embed_bwd workspace: same key), or None.  Once it
    exists EVERY embed_bwd into `dtable` marks the rows it writes (live[id] = 1; never cleared), so it holds "every id any batch has
    used so far" -- what the optimizer's row-aware pass steps (adam_step_ranges with rows).  The table outlives a workspace that had to
    grow (recordings and range tables bake its address, and a mark stays true for ever); a NEW table starts at zero and is only true
    after embed_live_rebuild -- its creator's job (trainer.FusedAdam.live_refresh)."""
    key = (dtable.shape[0], dtable.device, dtable.data_ptr())
    live = _embed_live.get(key)
    if live is None and create:
        live = _embed_live[key] = torch.zeros(dtable.shape[0], dtype=torch.uint8, device=dtable.device)
    return live


def embed_live_rebuild(live, exp_avg_rows, exp_avg_sq_rows, grad_rows=None):
    """live[r] = any bit set in row r of the moment tables (and the gradient table when given), fp32 [V, d] contiguous."""
    V, d = exp_avg_rows.shape
    assert live.numel() >= V and live.dtype == torch.uint8
    for t in (exp_avg_rows, exp_avg_sq_rows, grad_rows):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (V, d))
    L.check(L.load().vct_embed_live_rebuild(V, d, L.ptr(grad_rows), exp_avg_rows.data_ptr(), exp_avg_sq_rows.data_ptr(), live.data_ptr(),
                                            L.stream_ptr()), "vct_embed_live_rebuild")


def embed_bwd(ids, S, pad_id, dx, dtable, dropout: Drop = None, id_ws=None, exclusive: bool = False, on_grow=None, live=None):
    """dtable fp32 [V, d] = deterministic scatter-add of the dx rows.  exclusive=True: the caller guarantees that nothing but
    this function writes `dtable` between calls (the single-GPU fast training path: gradients are overwritten every step, never
    accumulated or averaged in place) -- from the second exclusive call on, only the rows the previous call wrote are zeroed
    (10 MB at cfg-B) instead of all V (62.5 MB).  Any non-exclusive call falls back to the full zero-fill and breaks the chain.
    live: uint8 [V] row table to mark (default: the one registered for `dtable`, embed_live_table)."""
    B = ids.shape[0]
    s, site, p = _drop(dropout)
    V = dtable.shape[0]
    incremental = False
    if live is None:
        live = embed_live_table(dtable)
    else:
        assert live.dtype == torch.uint8 and live.numel() >= V
    if id_ws is None:
        # one workspace per gradient table: it remembers the ids of the LAST call into that table (what the next incremental call
        # zeroes) -- shared between two models it made a replayed step of one zero the rows of the other's batch
        key = (V, dx.device, dtable.data_ptr())
        ent = _embed_ws.get(key)
        need = 2 * V + 4 + max(B * S, 65536)
        if ent is None or ent[0].numel() < need:
            # [first_pos V | count V | header 4 (positions of the last call) | ids in position order N]; room
            # for 65536 positions up front (recordings bake its address); an outgrown one stays alive for the recordings that use it
            if ent is not None:
                _embed_ws_retired.append(ent[0])
                # recordings made against the old workspace carry incremental = 1 and ITS "previous ids": replayed after a step on
                # the new workspace they would zero the wrong rows -> the owner drops them (engine: ctx.generation += 1)
                if on_grow is not None:
                    on_grow()
            ent = _embed_ws[key] = [torch.zeros(need, dtype=torch.int32, device=dx.device), None]
        id_ws = ent[0]
        incremental = exclusive and ent[1] == dtable.data_ptr()
        ent[1] = dtable.data_ptr() if exclusive else None
    else:
        assert id_ws.numel() >= 2 * V + 4 + B * S
    L.check(L.load().vct_embed_bwd_live(L.dtype_code(dx.dtype), B, S, dx.shape[1], V, ids.data_ptr(),
                                        ids.stride(0), int(pad_id), dx.data_ptr(), dtable.data_ptr(), id_ws.data_ptr(), id_ws.numel(),
                                        int(incremental), s, site, p, L.ptr(live), L.stream_ptr()), "vct_embed_bwd_live")


def sce_loss(logits, V, labels, S, pad_id, alpha, loss_out, dlogits, row_ws):
    """logits [N, ld>=V]; labels: int64 2-D view [B, >=S] whose first S columns are the targets."""
    N = logits.shape[0]
    L.check(L.load().vct_sce_loss(L.dtype_code(logits.dtype), N, S, V, logits.data_ptr(), _ld(logits), labels.data_ptr(),
                                  labels.stride(0), int(pad_id), float(alpha), loss_out.data_ptr(), L.ptr(dlogits),
                                  _ld(dlogits) if dlogits is not None else 0, row_ws.data_ptr(), L.stream_ptr()),
            "vct_sce_loss")
    return loss_out


def wce_loss(logits, V, labels, S, pad_id, seq_w, loss_out, dlogits, row_ws, tok_logp=None):
    """Sequence-weighted cross-entropy (include/vct_hip.h, vct_wce_loss).  logits [N, ld>=V]; labels: int64 2-D view [B, >=S] whose
    first S columns are the targets; seq_w: fp32 [N / S] on the device or None (all ones); dlogits: None = forward only;
    tok_logp: fp32 [N] or None."""
    N = logits.shape[0]
    if seq_w is not None:
        assert seq_w.dtype == torch.float32 and seq_w.is_contiguous() and seq_w.numel() * S == N, (seq_w.shape, N, S)
    if tok_logp is not None:
        assert tok_logp.dtype == torch.float32 and tok_logp.is_contiguous() and tok_logp.numel() == N
    L.check(L.load().vct_wce_loss(L.dtype_code(logits.dtype), N, S, V, logits.data_ptr(), _ld(logits), labels.data_ptr(),
                                  labels.stride(0), int(pad_id), L.ptr(seq_w), loss_out.data_ptr(), L.ptr(tok_logp), L.ptr(dlogits),
                                  _ld(dlogits) if dlogits is not None else 0, row_ws.data_ptr(), L.stream_ptr()),
            "vct_wce_loss")
    return loss_out


def group_sum(src, out, B: int, G: int, R: int):
    """out[g*R + r] = sum over n < G of src[(g*G + n)*R + r] (include/vct_hip.h, vct_group_sum): src [B*G*R, d], out [B*R, d],
    contiguous, same dtype."""
    d = src.shape[1]
    assert src.is_contiguous() and out.is_contiguous() and src.dtype == out.dtype
    assert tuple(src.shape) == (B * G * R, d) and tuple(out.shape) == (B * R, d), (src.shape, out.shape, B, G, R)
    L.check(L.load().vct_group_sum(L.dtype_code(src.dtype), B, G, R, d, src.data_ptr(), out.data_ptr(), L.stream_ptr()), "vct_group_sum")
    return out


def check_cider_ids(ids, device=None):
    """The refusals of ops.cider_d's candidate table, before any launch: int64 [B, N, L] on the GPU (on `device` when given),
    1 <= L <= 1 + VCT_CIDER_MAX_LEN columns (column 0 is the start token)."""
    if not torch.is_tensor(ids) or ids.dtype != torch.int64 or ids.dim() != 3:
        raise ValueError(f"cider_d: ids must be an int64 tensor [B, N, L], got {getattr(ids, 'dtype', type(ids))} {tuple(getattr(ids, 'shape', ()))}")
    if not ids.is_cuda or (device is not None and ids.device != device):
        raise ValueError(f"cider_d: ids must live on the reward tables' device, got {ids.device}")
    B, N, Lc = ids.shape
    if B < 1 or N < 1 or Lc < 1 or Lc > 1 + L.CIDER_MAX_LEN:
        raise ValueError(f"cider_d: ids [B >= 1, N >= 1, 1 <= L <= {1 + L.CIDER_MAX_LEN}] (start column + at most {L.CIDER_MAX_LEN} "
                         f"tokens), got {tuple(ids.shape)}")


def cider_d(ids, vid_rows, tab, out=None):
    """CIDEr-D of sampled ids on the device (include/vct_hip.h, vct_cider_d).  ids: int64 [B, N, L] (any strides, column 0 the
    start token); vid_rows: int32 [B] table rows; tab: rewards.DeviceCiderD (its device tensors `t` and scalars); out: fp32
    [B, N] contiguous or None (allocated).  Returns out.  Enqueued on the current stream; no host synchronisation."""
    check_cider_ids(ids)
    B, N, Lc = ids.shape
    if vid_rows.dtype != torch.int32 or tuple(vid_rows.shape) != (B,) or not vid_rows.is_contiguous() or vid_rows.device != ids.device:
        raise ValueError(f"cider_d: vid_rows must be int32 [B = {B}] on {ids.device}, got {vid_rows.dtype} {tuple(vid_rows.shape)} on {vid_rows.device}")
    if not 1 <= int(tab.n) <= L.CIDER_MAX_ORDER:
        raise ValueError(f"cider_d: n-gram orders 1 .. {L.CIDER_MAX_ORDER}, got n = {tab.n}")
    if out is None:
        out = torch.empty(B, N, dtype=torch.float32, device=ids.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (B, N) or not out.is_contiguous() or out.device != ids.device:
        raise ValueError(f"cider_d: out must be contiguous fp32 [{B}, {N}] on {ids.device}, got {out.dtype} {tuple(out.shape)}")
    t = tab.t
    if t["table_keys"].device != ids.device:
        raise ValueError(f"cider_d: the reward tables live on {t['table_keys'].device}, ids on {ids.device}")
    d = L.CiderDesc()
    d.B, d.N, d.L, d.n = B, N, Lc - 1, int(tab.n)
    d.ids = ids.data_ptr()
    d.stride_b, d.stride_n, d.stride_l = ids.stride(0), ids.stride(1), ids.stride(2)
    d.end_id, d.log_nvid, d.two_sigma_sq = int(tab.end_id), float(tab.log_nvid), float(tab.two_sigma_sq)
    d.vid_rows, d.n_videos, d.table_cap = vid_rows.data_ptr(), int(tab.n_videos), int(tab.table_cap)
    for k in ("table_keys", "table_idf", "vid_ref_ptr", "ref_len", "ref_norm", "ref_ent_ptr", "ent_keys", "ent_w"):
        setattr(d, k, t[k].data_ptr())
    d.reward = out.data_ptr()
    L.check(L.load().vct_cider_d(d, L.stream_ptr()), "vct_cider_d")
    return out


def scst_advantages(rewards, baseline=None, adv=None, base_out=None, means=None):
    """Advantages of sampled captions on the device (include/vct_hip.h, vct_scst_advantages).  rewards: fp32 [B, N] contiguous;
    baseline: fp32 [B] (e.g. the greedy captions' rewards) or None = the leave-one-out mean of the video's other samples
    (needs N >= 2).  Returns (adv fp32 [B * N] in seq_w's layout, base_out fp32 [B], means fp32 [2] = mean reward, mean baseline);
    each may be passed in (adv may be rewards' own storage)."""
    if not torch.is_tensor(rewards) or rewards.dtype != torch.float32 or rewards.dim() != 2 or not rewards.is_cuda or not rewards.is_contiguous():
        raise ValueError(f"scst_advantages: rewards must be contiguous fp32 [B, N] on the GPU, got {getattr(rewards, 'dtype', type(rewards))} "
                         f"{tuple(getattr(rewards, 'shape', ()))}")
    B, N = rewards.shape
    if B < 1 or N < 1:
        raise ValueError(f"scst_advantages: rewards [B >= 1, N >= 1], got {tuple(rewards.shape)}")
    if baseline is None and N < 2:
        raise ValueError("scst_advantages: the leave-one-out baseline needs num_samples >= 2")

    def buf(x, shape, what):
        if x is None:
            return torch.empty(shape, dtype=torch.float32, device=rewards.device)
        if x.dtype != torch.float32 or x.numel() != shape[0] or not x.is_contiguous() or x.device != rewards.device:
            raise ValueError(f"scst_advantages: {what} must be contiguous fp32 with {shape[0]} elements on {rewards.device}, "
                             f"got {x.dtype} {tuple(x.shape)} on {x.device}")
        return x
    if baseline is not None:
        baseline = buf(baseline, (B,), "baseline")
    adv, base_out, means = buf(adv, (B * N,), "adv"), buf(base_out, (B,), "base_out"), buf(means, (2,), "means")
    L.check(L.load().vct_scst_advantages(B, N, rewards.data_ptr(), L.ptr(baseline), adv.data_ptr(), base_out.data_ptr(), means.data_ptr(),
                                         L.stream_ptr()), "vct_scst_advantages")
    return adv, base_out, means


def check_capmetric_ids(ids, device=None):
    """The refusals of the caption-metric kernels' candidate table, before any launch: int64 [C, L] on the GPU (on `device` when
    given), 1 <= L <= 1 + VCT_CIDER_MAX_LEN columns (column 0 is the start token)."""
    if not torch.is_tensor(ids) or ids.dtype != torch.int64 or ids.dim() != 2:
        raise ValueError(f"capmetric: ids must be an int64 tensor [C, L], got {getattr(ids, 'dtype', type(ids))} {tuple(getattr(ids, 'shape', ()))}")
    if not ids.is_cuda or (device is not None and ids.device != device):
        raise ValueError(f"capmetric: ids must live on the metric tables' device, got {ids.device}")
    Cn, Lc = ids.shape
    if Cn < 1 or Lc < 1 or Lc > 1 + L.CIDER_MAX_LEN:
        raise ValueError(f"capmetric: ids [C >= 1, 1 <= L <= {1 + L.CIDER_MAX_LEN}] (start column + at most {L.CIDER_MAX_LEN} tokens), "
                         f"got {tuple(ids.shape)}")


def _capmetric_out(x, shape, dtype, dev, what):
    if x is None:
        return torch.empty(shape, dtype=dtype, device=dev)
    if x.dtype != dtype or tuple(x.shape) != tuple(shape) or not x.is_contiguous() or x.device != dev:
        raise ValueError(f"{what} must be contiguous {dtype} {list(shape)} on {dev}, got {x.dtype} {tuple(x.shape)} on {x.device}")
    return x


def _capmetric_rows(ids, vid_rows, what):
    Cn = ids.shape[0]
    if (not torch.is_tensor(vid_rows) or vid_rows.dtype != torch.int32 or tuple(vid_rows.shape) != (Cn,) or not vid_rows.is_contiguous()
            or vid_rows.device != ids.device):
        raise ValueError(f"{what}: vid_rows must be contiguous int32 [C = {Cn}] on {ids.device}, got "
                         f"{getattr(vid_rows, 'dtype', type(vid_rows))} {tuple(getattr(vid_rows, 'shape', ()))}")


def capmetric_counts(ids, vid_rows, tab, counts=None, rouge=None):
    """Per-caption BLEU / ROUGE-L statistics on the device (include/vct_hip.h, vct_capmetric_counts).  ids: int64 [C, L] (any
    strides, column 0 the start token); vid_rows: int32 [C] table rows; tab: metrics.DeviceCaptionMetrics (its device tensors `t`,
    end_id, beta_sq, n_videos); counts int32 [C, 12] / rouge fp64 [C, 3]: contiguous or None (allocated).  Returns (counts, rouge).
    Enqueued on the current stream; no host synchronisation."""
    check_capmetric_ids(ids)
    _capmetric_rows(ids, vid_rows, "capmetric_counts")
    Cn, Lc = ids.shape
    t = tab.t
    if t["ref_tok"].device != ids.device:
        raise ValueError(f"capmetric_counts: the metric tables live on {t['ref_tok'].device}, ids on {ids.device}")
    if not float(tab.beta_sq) > 0.0:
        raise ValueError(f"capmetric_counts: beta_sq > 0, got {tab.beta_sq}")
    counts = _capmetric_out(counts, (Cn, L.CAPMETRIC_COUNT_COLS), torch.int32, ids.device, "capmetric_counts: counts")
    rouge = _capmetric_out(rouge, (Cn, 3), torch.float64, ids.device, "capmetric_counts: rouge")
    d = L.CapMetricDesc()
    d.C, d.L = Cn, Lc - 1
    d.ids, d.stride_c, d.stride_l = ids.data_ptr(), ids.stride(0), ids.stride(1)
    d.end_id, d.vid_rows, d.n_videos, d.beta_sq = int(tab.end_id), vid_rows.data_ptr(), int(tab.n_videos), float(tab.beta_sq)
    for k in ("vid_ref_ptr", "ref_tok_ptr", "ref_tok"):
        setattr(d, k, t[k].data_ptr())
    d.counts, d.rouge = counts.data_ptr(), rouge.data_ptr()
    L.check(L.load().vct_capmetric_counts(d, L.stream_ptr()), "vct_capmetric_counts")
    return counts, rouge


def cider_d_eval(ids, vid_rows, tab, out=None):
    """The evaluation CIDEr of decoded ids on the device (include/vct_hip.h, vct_cider_d_eval): ops.cider_d's score with the end
    token dropped, un-rounded.  ids: int64 [C, L] (any strides); vid_rows: int32 [C]; tab: as ops.cider_d's (device tensors `t`
    and the scalars n, end_id, log_nvid, two_sigma_sq, n_videos, table_cap); out: fp64 [C] contiguous or None.  Returns out."""
    check_capmetric_ids(ids)
    _capmetric_rows(ids, vid_rows, "cider_d_eval")
    Cn, Lc = ids.shape
    if not 1 <= int(tab.n) <= L.CIDER_MAX_ORDER:
        raise ValueError(f"cider_d_eval: n-gram orders 1 .. {L.CIDER_MAX_ORDER}, got n = {tab.n}")
    t = tab.t
    if t["table_keys"].device != ids.device:
        raise ValueError(f"cider_d_eval: the metric tables live on {t['table_keys'].device}, ids on {ids.device}")
    out = _capmetric_out(out, (Cn,), torch.float64, ids.device, "cider_d_eval: out")
    d = L.CiderDesc()
    d.B, d.N, d.L, d.n = Cn, 1, Lc - 1, int(tab.n)
    d.ids = ids.data_ptr()
    d.stride_b, d.stride_n, d.stride_l = ids.stride(0), 0, ids.stride(1)
    d.end_id, d.log_nvid, d.two_sigma_sq = int(tab.end_id), float(tab.log_nvid), float(tab.two_sigma_sq)
    d.vid_rows, d.n_videos, d.table_cap = vid_rows.data_ptr(), int(tab.n_videos), int(tab.table_cap)
    for k in ("table_keys", "table_idf", "vid_ref_ptr", "ref_len", "ref_norm", "ref_ent_ptr", "ent_keys", "ent_w"):
        setattr(d, k, t[k].data_ptr())
    d.reward = None
    L.check(L.load().vct_cider_d_eval(d, out.data_ptr(), L.stream_ptr()), "vct_cider_d_eval")
    return out


def capmetric_finish(counts, rouge, cider=None, out=None):
    """The corpus-level fold of the per-caption rows (include/vct_hip.h, vct_capmetric_finish).  counts int32 [C, 12], rouge fp64
    [C, 3], cider fp64 [C] or None; all contiguous on one GPU.  Returns out fp64 [8] = {Bleu_1..4, ROUGE_L, CIDEr, their sum with
    Bleu_4, C}.  Enqueued on the current stream; no host synchronisation."""
    if (not torch.is_tensor(counts) or counts.dtype != torch.int32 or counts.dim() != 2 or counts.shape[1] != L.CAPMETRIC_COUNT_COLS
            or not counts.is_cuda or not counts.is_contiguous() or counts.shape[0] < 1):
        raise ValueError(f"capmetric_finish: counts must be contiguous int32 [C >= 1, {L.CAPMETRIC_COUNT_COLS}] on the GPU, got "
                         f"{getattr(counts, 'dtype', type(counts))} {tuple(getattr(counts, 'shape', ()))}")
    Cn = counts.shape[0]
    if not torch.is_tensor(rouge):
        raise ValueError("capmetric_finish: rouge must be a tensor")
    _capmetric_out(rouge, (Cn, 3), torch.float64, counts.device, "capmetric_finish: rouge")
    if cider is not None:
        if not torch.is_tensor(cider):
            raise ValueError("capmetric_finish: cider must be a tensor or None")
        _capmetric_out(cider, (Cn,), torch.float64, counts.device, "capmetric_finish: cider")
    out = _capmetric_out(out, (8,), torch.float64, counts.device, "capmetric_finish: out")
    L.check(L.load().vct_capmetric_finish(Cn, counts.data_ptr(), rouge.data_ptr(), L.ptr(cider), out.data_ptr(), L.stream_ptr()),
            "vct_capmetric_finish")
    return out


def match_loss_workspace_bytes(B: int, Dt: int) -> int:
    """Bytes of caller-owned workspace ops.match_loss needs (include/vct_hip.h); raises for a shape the kernels do not take."""
    n = int(L.load().vct_match_loss_workspace_bytes(int(B), int(Dt)))
    if n <= 0:
        raise ValueError(f"matching loss: batch {B} x text dimension {Dt} is outside the kernels' range "
                         f"(1 <= batch <= 256, dimension a multiple of 4 up to 1024)")
    return n


def match_loss(text, vid, loss_out, workspace, *, kind: str = "CSL", temp=None, temp_kind: str = "none", dvid=None, dtemp=None, sim=None):
    """The contrastive video-text loss, forward and backward in one call (include/vct_hip.h, vct_match_loss).  text / vid fp32
    [B, Dt] row-major views; temp: fp32 device scalar for temp_kind 'exp' (CSL: sim * exp(temp)) / 'div' (CSL_WDS: sim / temp), None
    for 'none'; loss_out fp32 [1]; dvid fp32 [B, Dt] or None (forward only); dtemp fp32 [1] or None; sim fp32 [B, B] or None (the
    logits as the loss saw them); workspace: >= match_loss_workspace_bytes(B, Dt) bytes."""
    B, Dt = text.shape
    if tuple(vid.shape) != (B, Dt):
        raise ValueError(f"matching loss: text {tuple(text.shape)} and video {tuple(vid.shape)} features must have one shape (square batches)")
    for t in (text, vid, dvid, sim, loss_out, temp, dtemp):
        if t is not None and t.dtype != torch.float32:
            raise ValueError("matching loss: every operand is fp32")
    need = match_loss_workspace_bytes(B, Dt)
    d = L.MatchLossDesc()
    d.B, d.Dt, d.loss_kind, d.temp_kind = B, Dt, L.MATCH_LOSS[kind], L.MATCH_TEMP[temp_kind]
    d.text, d.ld_text, d.vid, d.ld_vid = text.data_ptr(), _ld(text), vid.data_ptr(), _ld(vid)
    d.temp, d.loss, d.dtemp = L.ptr(temp), loss_out.data_ptr(), L.ptr(dtemp)
    if dvid is not None:
        d.dvid, d.ld_dvid = dvid.data_ptr(), _ld(dvid)
    if sim is not None:
        if tuple(sim.shape) != (B, B):
            raise ValueError(f"matching loss: sim must be [{B}, {B}]")
        d.sim, d.ld_sim = sim.data_ptr(), _ld(sim)
    d.workspace, d.workspace_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
    if d.workspace_bytes < need:
        raise ValueError(f"matching loss: workspace of {d.workspace_bytes} bytes, {need} needed")
    L.check(L.load().vct_match_loss(L.C.byref(d), L.stream_ptr()), "vct_match_loss")
    return loss_out


def retrieval_workspace_bytes(Nt: int, Nv: int, Dt: int, mode: str = "plain") -> int:
    """Bytes of caller-owned workspace ops.retrieval_ranks needs (include/vct_hip.h); raises for a shape the kernels do not take."""
    if mode not in L.RETRIEVAL_MODE:
        raise ValueError(f"retrieval: mode {mode!r}: 'plain' or 'dual_softmax'")
    n = int(L.load().vct_retrieval_workspace_bytes(int(Nt), int(Nv), int(Dt), L.RETRIEVAL_MODE[mode]))
    if n <= 0:
        raise ValueError(f"retrieval: {Nt} texts x {Nv} videos x dimension {Dt} is outside the kernels' range "
                         f"(1 <= texts, videos <= 2^20, dimension a multiple of 4 up to 1024)")
    return n


def retrieval_ranks(text, vid, gt, ranks_t2v, ranks_v2t, out, workspace, *, mode: str = "plain", tau=None, phases=None):
    """Text->video and video->text ranks over a whole split and their statistics (include/vct_hip.h, vct_retrieval_ranks).  text
    fp32 [Nt, Dt] / vid fp32 [Nv, Dt] row-major views (row stride a multiple of 4), gt int32 [Nt]; ranks_t2v int32 [Nt], ranks_v2t
    int32 [Nv], out fp64 [12]; tau: fp32 device scalar, required exactly for mode 'dual_softmax'; workspace: >=
    retrieval_workspace_bytes(Nt, Nv, Dt, mode) bytes; phases: None (everything) or an iterable of _lib.RETRIEVAL_PHASE names."""
    if mode not in L.RETRIEVAL_MODE:
        raise ValueError(f"retrieval: mode {mode!r}: 'plain' or 'dual_softmax'")
    if (mode == "dual_softmax") != (tau is not None):
        raise ValueError("retrieval: tau (an fp32 device scalar) is required for mode 'dual_softmax' and only for it")
    if text.dim() != 2 or vid.dim() != 2 or text.shape[1] != vid.shape[1]:
        raise ValueError(f"retrieval: text [Nt, Dt] and video [Nv, Dt] features expected, got {tuple(text.shape)} and {tuple(vid.shape)}")
    Nt, Dt = text.shape
    Nv = vid.shape[0]
    for t in (text, vid, tau):
        if t is not None and t.dtype != torch.float32:
            raise ValueError("retrieval: text, vid and tau are fp32")
    if text.stride(1) != 1 or vid.stride(1) != 1:
        raise ValueError("retrieval: text and vid rows must be contiguous")
    for t, n, what in ((gt, Nt, "gt"), (ranks_t2v, Nt, "ranks_t2v"), (ranks_v2t, Nv, "ranks_v2t")):
        if t.dtype != torch.int32 or tuple(t.shape) != (n,) or not t.is_contiguous():
            raise ValueError(f"retrieval: {what} must be contiguous int32 [{n}], got {t.dtype} {tuple(t.shape)}")
    if out.dtype != torch.float64 or tuple(out.shape) != (12,) or not out.is_contiguous():
        raise ValueError("retrieval: out must be contiguous fp64 [12]")
    retrieval_workspace_bytes(Nt, Nv, Dt, mode)                    # (raises for a shape outside the kernels' range)
    d = L.RetrievalDesc()
    d.Nt, d.Nv, d.Dt, d.mode = Nt, Nv, Dt, L.RETRIEVAL_MODE[mode]
    d.text, d.ld_text, d.vid, d.ld_vid = text.data_ptr(), (text.stride(0) if Nt > 1 else max(Dt, text.stride(0))), vid.data_ptr(), \
        (vid.stride(0) if Nv > 1 else max(Dt, vid.stride(0)))
    d.gt, d.tau, d.ranks_t2v, d.ranks_v2t, d.out = gt.data_ptr(), L.ptr(tau), ranks_t2v.data_ptr(), ranks_v2t.data_ptr(), out.data_ptr()
    d.workspace, d.workspace_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
    d.phases = 0 if phases is None else sum(L.RETRIEVAL_PHASE[p] for p in set(phases))
    L.check(L.load().vct_retrieval_ranks(L.C.byref(d), L.stream_ptr()), "vct_retrieval_ranks")
    return out


def _agg_desc(t, B, Te):
    if t.dim() != 2 or t.shape[0] != B * Te or not t.is_contiguous():
        raise ValueError(f"matching aggregation rows: contiguous [B*Te, d] = [{B * Te}, d] expected, got {tuple(t.shape)}")
    d = L.MatchAggDesc()
    d.dtype, d.B, d.Te, d.d = L.dtype_code(t.dtype), B, Te, t.shape[1]
    return d


def match_agg_fwd(mem, agg, B, Te):
    """agg fp32 [B, d] <- memory row b * Te of every sample (the aggregation row of stream 0; include/vct_hip.h, vct_match_agg_fwd)."""
    d = _agg_desc(mem, B, Te)
    if agg.dtype != torch.float32 or tuple(agg.shape) != (B, mem.shape[1]) or not agg.is_contiguous():
        raise ValueError("matching aggregation rows: agg must be contiguous fp32 [B, d]")
    d.mem, d.agg = mem.data_ptr(), agg.data_ptr()
    L.check(L.load().vct_match_agg_fwd(L.C.byref(d), L.stream_ptr()), "vct_match_agg_fwd")
    return agg


def match_agg_bwd(dmem, dagg, B, Te, beta: float, empty: bool = False):
    """dmem[b*Te + r] <- beta * dmem[b*Te + r] + (r == 0 ? (1 - beta) * dagg[b] : 0), in place over the whole [B*Te, d]; empty: dmem
    holds nothing yet and is not read (include/vct_hip.h, vct_match_agg_bwd)."""
    d = _agg_desc(dmem, B, Te)
    if dagg.dtype != torch.float32 or tuple(dagg.shape) != (B, dmem.shape[1]) or not dagg.is_contiguous():
        raise ValueError("matching aggregation rows: dagg must be contiguous fp32 [B, d]")
    d.dmem, d.dagg, d.beta, d.empty = dmem.data_ptr(), dagg.data_ptr(), float(beta), int(bool(empty))
    L.check(L.load().vct_match_agg_bwd(L.C.byref(d), L.stream_ptr()), "vct_match_agg_bwd")
    return dmem


def scale(x: torch.Tensor, s: float):
    """x *= s over a contiguous fp32 range (include/vct_hip.h, vct_scale)."""
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError("scale: a contiguous fp32 tensor")
    L.check(L.load().vct_scale(x.data_ptr(), x.numel(), float(s), L.stream_ptr()), "vct_scale")
    return x


def axpby(out: torch.Tensor, x: torch.Tensor, a: float, y: Optional[torch.Tensor] = None, b: float = 0.0):
    """out = a * x + b * y over contiguous fp32 tensors of one size (y None: a * x; include/vct_hip.h, vct_axpby)."""
    for t in (out, x, y):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != out.numel()):
            raise ValueError("axpby: contiguous fp32 tensors of one size")
    L.check(L.load().vct_axpby(out.data_ptr(), x.data_ptr(), float(a), L.ptr(y), float(b), out.numel(), L.stream_ptr()), "vct_axpby")
    return out


def warm(t: torch.Tensor):
    """Read-only pass over a tensor: pulls it into the memory-side cache for the launch that streams it next (include/vct_hip.h, vct_warm)."""
    L.check(L.load().vct_warm(t.data_ptr(), t.numel() * t.element_size(), L.stream_ptr()), "vct_warm")


def cast(src, dst):
    L.check(L.load().vct_cast(L.dtype_code(src.dtype), L.dtype_code(dst.dtype), src.data_ptr(), dst.data_ptr(),
                              src.numel(), L.stream_ptr()), "vct_cast")
    return dst


def argmax_rows(x, out, cols=None):
    """out: int64 1-D tensor (any stride): out[row] = first index of the row maximum."""
    L.check(L.load().vct_argmax_rows(L.dtype_code(x.dtype), x.shape[0], cols or x.shape[1], x.data_ptr(), _ld(x),
                                     out.data_ptr(), out.stride(0), L.stream_ptr()), "vct_argmax_rows")
    return out


def advance_seed(seed):
    L.check(L.load().vct_advance_seed(seed.data_ptr(), L.stream_ptr()), "vct_advance_seed")


def adam_step(param, grad, exp_avg, exp_avg_sq, shadow, lr, beta1, beta2, eps, weight_decay, step_dev, skip=(0, 0), bump=True,
              hyper=None, pack=None):
    """Fused Adam/AdamW over flat fp32 buffers (+ bf16 shadow refresh).  step_dev: int32[1] device counter.
    `param` may be a slice of the flat buffer (range-by-range stepping): pass the same slice of every buffer,
    `skip` relative to the slice start, bump=False, and finish with adam_bump(step_dev).  hyper: device fp32 [5]
    (lr, beta1, beta2, eps, weight_decay) read by the kernel instead of the scalars (graph / launch-list replays)."""
    if pack is not None:      # (device table of vct_adam_pack_seg, entries, flat index of param[0]): packed weight copies written in the same pass
        table, nseg, base = pack
        L.check(L.load().vct_adam_step_pk(param.data_ptr(), grad.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(), L.ptr(shadow),
                                          param.numel(), float(lr), float(beta1), float(beta2), float(eps), float(weight_decay),
                                          step_dev.data_ptr(), int(skip[0]), int(skip[1]), int(bool(bump)), L.ptr(hyper),
                                          table.data_ptr(), int(nseg), int(base), L.stream_ptr()), "vct_adam_step_pk")
        return
    L.check(L.load().vct_adam_step(param.data_ptr(), grad.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(), L.ptr(shadow),
                                   param.numel(), float(lr), float(beta1), float(beta2), float(eps), float(weight_decay),
                                   step_dev.data_ptr(), int(skip[0]), int(skip[1]), int(bool(bump)), L.ptr(hyper), L.stream_ptr()),
            "vct_adam_step")


def adam_ranges_table(ranges, device, rows=None):
    """Device table for adam_step_ranges: ranges = sorted [(begin, end, has_shadow)] of flat elements (multiples of 4).
    Returns (table tensor, entries, workgroups).  rows = {range index: (origin, row_len, nrows, live uint8 tensor)}: those ranges lie
    inside a row-major table (row 0 at flat element `origin`) with a per-row live table, and the pass skips the rows that are not
    live (include/vct_hip.h, vct_adam_rows); the result then carries the device row table (and the live tensors) behind the three."""
    EPB = 4096
    arr = (L.AdamRange * len(ranges))()
    blk = 0
    for i, (a, b, sh) in enumerate(ranges):
        assert a % 4 == 0 and b % 4 == 0 and b > a
        arr[i].begin, arr[i].end, arr[i].blk0, arr[i].shadow = int(a), int(b), blk, int(bool(sh))
        blk += (b - a + EPB - 1) // EPB
    table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(device)
    if not rows:
        return table, len(ranges), blk
    rarr = (L.AdamRows * len(ranges))()
    for i, (origin, row_len, nrows, live) in rows.items():
        assert 0 <= i < len(ranges) and not ranges[i][2], "a range with a bf16 shadow is stepped densely: give it no row table"
        assert row_len > 0 and row_len % 4 == 0 and origin % 4 == 0 and live.dtype == torch.uint8 and live.numel() >= nrows
        rarr[i].origin, rarr[i].row_len, rarr[i].nrows, rarr[i].live = int(origin), int(row_len), int(nrows), live.data_ptr()
    rtable = torch.frombuffer(bytearray(bytes(rarr)), dtype=torch.uint8).to(device)
    return table, len(ranges), blk, rtable, [r[3] for r in rows.values()]


def adam_step_ranges(param, grad, exp_avg, exp_avg_sq, shadow, table, lr, beta1, beta2, eps, weight_decay, step_dev, hyper=None, pack=None):
    """vct_adam_step over a LIST of ranges of the WHOLE flat buffers in one launch (table from adam_ranges_table): what is left for a
    separate pass when the weight matrices are stepped inside their weight-gradient GEMMs.  pack = (device table of
    vct_adam_pack_seg with flat indices, entries) or None.  No step-counter bump.  A table built with rows skips the rows that are
    not live (same bits: a skipped row is one the update would not change)."""
    tab, n, blocks = table[:3]
    pk, nseg = (pack[0].data_ptr(), int(pack[1])) if pack is not None and pack[1] else (0, 0)
    if len(table) > 3:
        L.check(L.load().vct_adam_step_ranges_rows(param.data_ptr(), grad.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(),
                                                   L.ptr(shadow), tab.data_ptr(), int(n), int(blocks), float(lr), float(beta1),
                                                   float(beta2), float(eps), float(weight_decay), step_dev.data_ptr(), L.ptr(hyper), pk,
                                                   nseg, table[3].data_ptr(), L.stream_ptr()), "vct_adam_step_ranges_rows")
        return
    L.check(L.load().vct_adam_step_ranges(param.data_ptr(), grad.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(), L.ptr(shadow),
                                          tab.data_ptr(), int(n), int(blocks), float(lr), float(beta1), float(beta2), float(eps),
                                          float(weight_decay), step_dev.data_ptr(), L.ptr(hyper), pk, nseg, L.stream_ptr()),
            "vct_adam_step_ranges")


def adam_step_2d(param, grad, exp_avg, exp_avg_sq, shadow, shadow_t, lr, beta1, beta2, eps, weight_decay, step_dev, hyper=None):
    """vct_adam_step on one 2-D weight (views [rows, cols] of the flat buffers) that also writes the transposed bf16 shadow
    shadow_t [cols, ld >= rows] in the same pass."""
    rows, cols = param.shape
    L.check(L.load().vct_adam_step_2d(param.data_ptr(), grad.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(), L.ptr(shadow),
                                      shadow_t.data_ptr(), rows, cols, shadow_t.stride(0), float(lr), float(beta1), float(beta2),
                                      float(eps), float(weight_decay), step_dev.data_ptr(), L.ptr(hyper), L.stream_ptr()),
            "vct_adam_step_2d")


def adam_bump(step_dev):
    L.check(L.load().vct_adam_step(step_dev.data_ptr(), step_dev.data_ptr(), step_dev.data_ptr(), step_dev.data_ptr(), 0, 0,
                                   0.0, 0.0, 0.0, 0.0, 0.0, step_dev.data_ptr(), 0, 0, 1, 0, L.stream_ptr()), "vct_adam_step(bump)")


def greedy_select(x, out, end_id: int, ended, ended_count, all_ended_at, t: int, cols=None):
    """argmax_rows into `out` (column t of the id matrix) + the decode loop's end-of-sequence bookkeeping, one launch."""
    L.check(L.load().vct_greedy_select(L.dtype_code(x.dtype), x.shape[0], cols or x.shape[1], x.data_ptr(), _ld(x),
                                       out.data_ptr(), out.stride(0), int(end_id), ended.data_ptr(), ended_count.data_ptr(),
                                       all_ended_at.data_ptr(), int(t), L.stream_ptr()), "vct_greedy_select")
    return out


def beam_select_workspace_bytes(dtype, B: int, K: int, V: int) -> int:
    """Workspace of vct_beam_select (include/vct_hip.h): chunk partials of every row."""
    chunk = 256 * (8 if dtype == torch.bfloat16 else 4)
    return B * K * ((V + chunk - 1) // chunk) * (2 + 2 * K) * 4


def beam_select(x, B: int, K: int, scores, finished, parent, out, end_id: int, pad_id: int, finished_count, all_finished_at,
                t: int, ws, cols=None):
    """One beam-search selection step (include/vct_hip.h, vct_beam_select): the K best continuations of each video's K beams
    -> parent rows, tokens into `out` (column t of the token table), scores / finished flags in place, stop bookkeeping."""
    L.check(L.load().vct_beam_select(L.dtype_code(x.dtype), int(B), int(K), int(cols or x.shape[1]), x.data_ptr(), _ld(x),
                                     scores.data_ptr(), finished.data_ptr(), parent.data_ptr(), out.data_ptr(), out.stride(0),
                                     int(end_id), int(pad_id), finished_count.data_ptr(), all_finished_at.data_ptr(), int(t),
                                     ws.data_ptr(), ws.numel() * ws.element_size(), L.stream_ptr()), "vct_beam_select")


def beam_reorder(src, dst, parent, M: int, Lmax: int, d: int, t: int):
    """Slots < t of every layer's self-attention cache follow their beam's parent row (vct_beam_reorder): src / dst [L, M * Lmax, 3d]."""
    L.check(L.load().vct_beam_reorder(L.dtype_code(src.dtype), src.shape[0], int(M), int(Lmax), int(d), int(t), parent.data_ptr(),
                                      src.data_ptr(), dst.data_ptr(), src.stride(0), L.stream_ptr()), "vct_beam_reorder")


def sample_select_workspace_bytes(dtype, rows: int, V: int) -> int:
    """Workspace of vct_sample_select (include/vct_hip.h): chunk partials of every row, sized for the largest k (64)."""
    chunk = 256 * (8 if dtype == torch.bfloat16 else 4)
    return rows * ((V + chunk - 1) // chunk) * (2 + 2 * 64) * 4


def sample_select(x, out, end_id: int, pad_id: int, ended, ended_count, all_ended_at, t: int, step_logp, seq_logp, ctl, ws, cols=None):
    """One sampled selection step (include/vct_hip.h, vct_sample_select): a token per row drawn from softmax(x * inv_temp) over
    the row's top-k / nucleus candidates -> `out` (column t of the id table), step_logp written, seq_logp +=, greedy's end
    bookkeeping.  ctl: the 16-byte device control block {uint32 seed, int32 top_k, float inv_temp, float top_p}."""
    d = L.SampleSelectDesc()
    d.dtype, d.rows, d.V, d.t = L.dtype_code(x.dtype), x.shape[0], int(cols or x.shape[1]), int(t)
    d.x, d.ldx, d.out, d.out_stride = x.data_ptr(), _ld(x), out.data_ptr(), out.stride(0)
    d.end_id, d.pad_id = int(end_id), int(pad_id)
    d.ended, d.ended_count, d.all_ended_at = ended.data_ptr(), ended_count.data_ptr(), all_ended_at.data_ptr()
    d.step_logp, d.seq_logp, d.ctl = step_logp.data_ptr(), seq_logp.data_ptr(), ctl.data_ptr()
    d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel() * ws.element_size()
    L.check(L.load().vct_sample_select(L.C.byref(d), L.stream_ptr()), "vct_sample_select")


def decode_gemv(W, out, B, *, bias=None, pro="none", x_in=None, ln1=None, ln2=None, embed=None, attn=None, act=None, res=None,
                out_native=False, ld_out=None, x_out=None, n_valid=None):
    """One stage of the small-batch greedy-decode step (include/vct_hip.h, vct_decode_gemv).  W [N, K]; out: tensor whose row b starts
    at out.data_ptr() + b*ld_out elements.  embed = (ids view [B] (any stride), table fp32, pos_row fp32 [K]);
    attn = (q view [B, K], k view, v view, kv_ld, kv_bs, H, Lk) -- all in W's dtype; ln1 / ln2 = (gamma, beta)."""
    d = L.DecodeGemvDesc()
    d.wdtype, d.B, d.N, d.K = L.dtype_code(W.dtype), B, (n_valid or W.shape[0]), W.shape[1]
    d.W, d.ldw, d.bias = W.data_ptr(), _ld(W), L.ptr(bias)
    d.pro, d.act = L.DEC_PRO[pro], L.ACT[act]
    if x_in is not None:
        d.x_in, d.ld_x = x_in.data_ptr(), x_in.stride(0)
    if ln1 is not None:
        d.g1, d.b1 = ln1[0].data_ptr(), ln1[1].data_ptr()
    if ln2 is not None:
        d.g2, d.b2 = ln2[0].data_ptr(), ln2[1].data_ptr()
    if embed is not None:
        ids, table, pos_row = embed
        d.ids, d.id_stride, d.table, d.pos_row = ids.data_ptr(), ids.stride(0), table.data_ptr(), pos_row.data_ptr()
    if attn is not None:
        q, k, v, kv_ld, kv_bs, H, Lk = attn
        d.q, d.q_bs, d.kc, d.vc, d.kv_ld, d.kv_bs, d.H, d.Lk = q.data_ptr(), q.stride(0), k.data_ptr(), v.data_ptr(), kv_ld, kv_bs, H, Lk
    if res is not None:
        d.res, d.ld_res = res.data_ptr(), res.stride(0)
    d.out, d.ld_out, d.out_native = out.data_ptr(), (ld_out if ld_out is not None else out.stride(0)), int(out_native)
    d.x_out = L.ptr(x_out)
    L.check(L.load().vct_decode_gemv(d, L.stream_ptr()), "vct_decode_gemv")


def decode_block(kind: str, d: int, *, w_a, b_a, part_out, embed=None, res=None, res_bias=None, part=None, ln1=None, ln2=None, x_out=None,
                 slot=None, kc=None, vc=None, kv_ld=0, Lk=1, w_b=None, ff=0, act=None, V=0, select=None):
    """One block of the batch-1 greedy-decode step (include/vct_hip.h, vct_decode_block): kind in {'self', 'cross', 'ffn', 'gen'}.
    embed = (id view [1] int64, table fp32 [V, d], pos_row fp32 [d]) or the vector res + res_bias + sum(part) (fp32 [d] / [n, d])."""
    q = L.DecodeBlockDesc()
    q.kind, q.d, q.ff, q.V, q.Lk, q.act = {"self": 0, "cross": 1, "ffn": 2, "gen": 3}[kind], d, ff, V, Lk, L.ACT[act]
    if embed is not None:
        ids, table, pos_row = embed
        q.id, q.table, q.pos_row = ids.data_ptr(), table.data_ptr(), pos_row.data_ptr()
    q.res, q.res_bias = L.ptr(res), L.ptr(res_bias)
    if part is not None:
        q.part, q.n_part = part.data_ptr(), part.shape[0]
    if ln1 is not None:
        q.g1, q.b1 = ln1[0].data_ptr(), ln1[1].data_ptr()
    if ln2 is not None:
        q.g2, q.b2 = ln2[0].data_ptr(), ln2[1].data_ptr()
    q.x_out = L.ptr(x_out)
    q.w_a, q.ld_a, q.b_a = w_a.data_ptr(), _ld(w_a), b_a.data_ptr()
    q.slot, q.kc, q.vc, q.kv_ld = L.ptr(slot), L.ptr(kc), L.ptr(vc), kv_ld
    if w_b is not None:
        q.w_b, q.ld_b = w_b.data_ptr(), _ld(w_b)
    q.part_out = part_out.data_ptr()
    if select is not None:      # kind 'gen': (sel_ws fp32 [2 * ceil(V / 128) + 1] zeroed, out id view [1], end_id, ended, ended_count, all_ended_at, t)
        ws, out, end_id, ended, ended_count, all_ended_at, t = select
        assert ws.numel() >= 2 * ((V + 127) // 128) + 1
        q.sel_ws, q.tok_out, q.end_id, q.ended = ws.data_ptr(), out.data_ptr(), int(end_id), ended.data_ptr()
        q.ended_count, q.all_ended_at, q.t = ended_count.data_ptr(), all_ended_at.data_ptr(), int(t)
    L.check(L.load().vct_decode_block(q, L.stream_ptr()), "vct_decode_block")


_db_ok = {}


def decode_block_supported(dtype, d: int, H: int, ff: int, Lk: int) -> bool:
    if dtype != torch.bfloat16:
        return False
    key = (d, H, ff, Lk)
    r = _db_ok.get(key)
    if r is None:
        r = _db_ok[key] = bool(L.load().vct_decode_block_supported(L.BF16, d, H, ff, Lk))
    return r


def transpose(src: torch.Tensor, dst: torch.Tensor):
    """dst[c, r] = src[r, c] (bf16; row strides free)."""
    L.check(L.load().vct_transpose(L.dtype_code(src.dtype), src.shape[0], src.shape[1], src.data_ptr(), src.stride(0),
                                   dst.data_ptr(), dst.stride(0), L.stream_ptr()), "vct_transpose")
    return dst


def decode_linear(W, out, *, x=None, x_pre=None, ln=None, x_norm=None, bias=None, act=None, res=None, n_valid=None, embed=None):
    """One nn.Linear of the batched greedy-decode step on the M <= 256 rows of the current position (include/vct_hip.h,
    vct_decode_linear): out = act(in W^T + bias) + res with in = x (bf16 rows) or LayerNorm(x_pre; *ln) of fp32 pre-norm rows
    (x_norm: fp32 buffer that receives the normalised rows), or the embedded token rows: embed = (ids view [M] (any stride),
    table fp32 [V, K], pos_row fp32 [K]).  out / res: row views (any row stride)."""
    d = L.DecodeLinearDesc()
    d.M, d.N, d.K = out.shape[0], (n_valid or W.shape[0]), W.shape[1]
    d.out_dtype, d.act = L.dtype_code(out.dtype), L.ACT[act]
    if x is not None:
        d.x, d.ldx = x.data_ptr(), x.stride(0)
    if x_pre is not None:
        d.x_pre, d.ld_pre = x_pre.data_ptr(), x_pre.stride(0)
        d.ln_g, d.ln_b = ln[0].data_ptr(), ln[1].data_ptr()
    if embed is not None:
        ids, table, pos_row = embed
        d.x_pre, d.ld_pre, d.ln_b = table.data_ptr(), table.stride(0), pos_row.data_ptr()
        d.ids, d.id_stride = ids.data_ptr(), ids.stride(0)
    if x_norm is not None:
        d.x_norm, d.ld_norm = x_norm.data_ptr(), x_norm.stride(0)
    d.W, d.ldw, d.bias = W.data_ptr(), _ld(W), L.ptr(bias)
    if res is not None:
        d.res, d.ld_res, d.res_dtype = res.data_ptr(), res.stride(0), L.dtype_code(res.dtype)
    d.out, d.ldo = out.data_ptr(), out.stride(0)
    L.check(L.load().vct_decode_linear(d, L.stream_ptr()), "vct_decode_linear")
    return out


def decode_ln2(x, ln1, ln2, y):
    """y (bf16 [M, K]) = LayerNorm(LayerNorm(x; *ln1); *ln2) of fp32 rows; ln2 = None: one LayerNorm."""
    g2, b2 = (ln2[0].data_ptr(), ln2[1].data_ptr()) if ln2 is not None else (None, None)
    L.check(L.load().vct_decode_ln2(x.shape[0], x.shape[1], x.data_ptr(), x.stride(0), ln1[0].data_ptr(), ln1[1].data_ptr(), g2, b2,
                                    y.data_ptr(), y.stride(0), L.stream_ptr()), "vct_decode_ln2")
    return y


def gather_pad_rows(store: torch.Tensor, offsets: torch.Tensor, idx: torch.Tensor, tmax: int, out_dtype=torch.float32):
    """store fp32 [rows, E] (packed clips), offsets int64 [n+1], idx int64 [B] -> (feat [B, tmax, E], mask bool [B, tmax])."""
    B, E = idx.numel(), store.shape[1]
    out = torch.empty(B, tmax, E, dtype=out_dtype, device=store.device)
    mask = torch.empty(B, tmax, dtype=torch.bool, device=store.device)
    L.check(L.load().vct_gather_pad_rows(L.dtype_code(out_dtype), B, tmax, E, store.data_ptr(), offsets.data_ptr(), idx.data_ptr(),
                                         out.data_ptr(), mask.data_ptr(), L.stream_ptr()), "vct_gather_pad_rows")
    return out, mask


# ---- host runtime (csrc/vct_runtime.hip): cross-stream ordering, launch lists, live timing ----------------------------
def _sptr(stream) -> int:
    return stream.cuda_stream if stream is not None else L.stream_ptr()


def stream_wait(waiter, signal):
    """`waiter` (torch stream, None = current) waits for everything enqueued so far on `signal`.  Recordable."""
    L.check(L.load().vct_stream_wait(_sptr(waiter), _sptr(signal)), "vct_stream_wait")


def sync_record(ident: int, stream=None):
    L.check(L.load().vct_sync_record(int(ident), _sptr(stream)), "vct_sync_record")


def sync_wait(ident: int, stream=None):
    L.check(L.load().vct_sync_wait(int(ident), _sptr(stream)), "vct_sync_wait")


import threading

_rec = threading.local()     # .ll = the LaunchList recording on THIS thread (the C recorder is thread_local too): host-side collectives
                             # issued on another thread while this one records run immediately, as they must


def is_recording() -> bool:
    return getattr(_rec, "ll", None) is not None


_host_fns = []          # CFUNCTYPE objects of eager host calls made outside any recording (kept alive for the duration of the call only)


def host_call(fn, stream=None):
    """Run the Python callable `fn()` on the host once everything enqueued on `stream` (None = current) so far has finished --
    immediately, or at this point of every replay while a launch list records (include/vct_hip.h, vct_cmdlist_host_call).  For
    host-side collectives (torch.distributed / gloo) inside a recorded step; an exception in fn becomes status 1 of the replay."""
    def thunk(_arg):
        try:
            fn()
            return 0
        except Exception:                     # never unwind through the C frames of the replay loop
            import traceback
            traceback.print_exc()
            return 1
    cfn = L.HOST_FN(thunk)
    ll = getattr(_rec, "ll", None)
    if ll is not None:
        ll._thunks.append(cfn)            # the recording owns its thunks (and the tensors they capture): released with the list
    L.check(L.load().vct_cmdlist_host_call(L.C.cast(cfn, L.vp), None, _sptr(stream)), "vct_cmdlist_host_call")


def masked_stream(cu_bits, device=None):
    """torch stream restricted to the compute units whose indices are in `cu_bits` (iterable of ints < 256); an empty /
    None selection gives an ordinary stream.  Wraps vct_stream_create_masked; the stream lives as long as the process."""
    words = (L.u32 * 8)()
    n = 0
    for c in (cu_bits or ()):
        words[c // 32] |= (1 << (c % 32))
        n += 1
    h = L.vp()
    L.check(L.load().vct_stream_create_masked(words, 8 if n else 0, L.C.byref(h)), "vct_stream_create_masked")
    return torch.cuda.ExternalStream(h.value, device=device)


TAPS = {"gen_fwd": 0, "gen_dx": 1, "gen_dw": 2, "layers_fwd": 3, "loss": 4, "adam": 5, "step": 6,
        # data-parallel exchange (trainer.ShardedExchange): what the compute stream WAITS for the communicator at the end of a step,
        # and how long each gradient bucket (reduce-scatter -> Adam on the shard -> all-gather -> cast) occupies the communicator's stream
        "comm_wait": 7, **{f"comm_b{i}": 8 + i for i in range(8)},
        # the two sample-stationary stack launches of the forward (encoder incl. its front end / decoder incl. the token embedding)
        "ss_enc": 16, "ss_dec": 17}
_taps_on = False
_taps_only = None        # None = every tag, else the set of tags that are bracketed


def taps_enable(on: bool, only=None):
    """Switch the live timing brackets on / off; `only`: an iterable of tags to restrict them to.  Every bracket is two HIP event
    records in the step's stream -- seven brackets cost the cfg-B step ~55 us (tools/taps_cost.py) -- so a benchmark keeps only the
    one it needs inside its timed region.  Recorded launch lists / graphs contain the brackets that were active when they were
    made: drop them (CaptionTrainer.drop_recordings) after changing this."""
    global _taps_on, _taps_only
    _taps_on = bool(on)
    _taps_only = None if only is None else frozenset(only)
    L.check(L.load().vct_tap_enable(int(_taps_on)), "vct_tap_enable")


def tap(tag: str, phase: int, stream=None):
    """Bracket a region of `stream` with HIP timing events (phase 0 = start, 1 = end); no-op while taps are disabled."""
    if _taps_on and (_taps_only is None or tag in _taps_only):
        L.check(L.load().vct_tap(TAPS[tag], phase, _sptr(stream)), "vct_tap")


def tap_collect(tag: str, cap: int = 4096):
    """Elapsed milliseconds of every bracket of `tag` executed since the last collect (waits for them)."""
    buf = (L.f32 * cap)()
    n = L.load().vct_tap_collect(TAPS[tag], buf, cap)
    if n < 0:
        L.check(n, "vct_tap_collect")
    return [float(buf[i]) for i in range(n)]


class LaunchList:
    """One recorded step: `with ll.record(): <issue the step>` captures every vct_* launch made on this thread (nothing
    executes), `ll.replay()` re-issues them from C.  Launches aimed at the stream that was current at record time go to
    the stream current at replay time."""

    def __init__(self):
        h = L.vp()
        L.check(L.load().vct_cmdlist_create(L.C.byref(h)), "vct_cmdlist_create")
        self._h = h
        self._thunks = []                 # host-call thunks of this recording (ops.host_call)

    class _Rec:
        def __init__(self, ll):
            self.ll = ll

        def __enter__(self):
            L.check(L.load().vct_cmdlist_begin(self.ll._h, L.stream_ptr()), "vct_cmdlist_begin")
            self.ll._thunks = []          # a re-recording replaces the commands, and with them the thunks they call
            _rec.ll = self.ll
            return self.ll

        def __exit__(self, *exc):
            _rec.ll = None
            L.check(L.load().vct_cmdlist_end(self.ll._h), "vct_cmdlist_end")
            return False

    def record(self):
        return LaunchList._Rec(self)

    def replay(self):
        L.check(L.load().vct_cmdlist_replay(self._h, L.stream_ptr()), "vct_cmdlist_replay")

    def __len__(self):
        return int(L.load().vct_cmdlist_size(self._h))

    @property
    def n_streams(self):
        return int(L.load().vct_cmdlist_streams(self._h))

    def close(self):
        if self._h is not None and self._h.value:
            L.load().vct_cmdlist_destroy(self._h)
            self._h = None
            self._thunks = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
