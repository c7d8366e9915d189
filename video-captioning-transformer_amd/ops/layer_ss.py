"""The sample-stationary layer stacks (csrc/vct_layer_ss.hip, csrc/vct_layer_ss_bwd.hip) and their packed weight streams."""
import torch

from .. import _lib as L

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
