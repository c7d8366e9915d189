"""Caption decoding: greedy / beam / sampled selection and the KV-cached decode-step kernels (csrc/vct_decode.hip,
csrc/vct_decode_block.hip, csrc/vct_select.hip, csrc/vct_beam.hip, csrc/vct_sample.hip over csrc/vct_select_core.h,
csrc/vct_logit_controls.hip, csrc/vct_ensemble.hip)."""
import torch

from .. import _lib as L
from ._common import _ld


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
    n = int(L.load().vct_sample_select_workspace_bytes(L.dtype_code(dtype), int(rows), int(V)))
    if n <= 0:
        raise ValueError(f"sample_select: {rows} rows x {V} columns of {dtype} is outside the kernels' range "
                         f"(fp32 or bf16, at least one row and one column)")
    return n


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


def logit_controls(x, ids, ended, ctl, t: int, end_id: int, cols=None, parents=None, K: int = 0):
    """The generation controls of one decode step (include/vct_hip.h, vct_logit_controls): repetition penalty, banned ids,
    minimum length and the no-repeat n-gram ban, in place on the logits x [rows, ldx] (columns < cols) of step t.  ids: the id
    matrix [rows, Lmax] int64 -- or, with parents (int32 [Lmax, rows], K beams per video), the beams' token table, whose
    histories follow the parent back-track.  ended: the session's ended / finished flags (bool or uint8 [rows]); ctl: the
    160-byte device control block (decode.GenerationControls.pack)."""
    d = L.LogitControlsDesc()
    d.dtype, d.rows, d.V, d.t = L.dtype_code(x.dtype), x.shape[0], int(cols or x.shape[1]), int(t)
    d.x, d.ldx, d.end_id = x.data_ptr(), _ld(x), int(end_id)
    d.ids, d.ids_stride, d.ended, d.ctl = ids.data_ptr(), ids.stride(0), ended.data_ptr(), ctl.data_ptr()
    if parents is not None:
        d.parents, d.parents_stride, d.K = parents.data_ptr(), parents.stride(0), int(K)
    L.check(L.load().vct_logit_controls(L.C.byref(d), L.stream_ptr()), "vct_logit_controls")
    return x


def ensemble_combine(xs, w, out, mode: str = "prob", cols=None):
    """The members' logits of one decode step -> one fp32 row of combined log-probabilities per row (include/vct_hip.h,
    vct_ensemble_combine).  xs: 1..8 tensors [rows, ld_m] (fp32 or bf16, mixed freely); w: DEVICE fp32 [8], normalised by the
    host (a member with weight 0 is skipped); out: fp32 [rows, ld_out]; mode "prob" (arithmetic mean of the probabilities) or
    "logp" (weighted sum of the log-probabilities).  Columns >= cols are neither read nor written."""
    if not 1 <= len(xs) <= L.ENSEMBLE_MAX:
        raise ValueError(f"ensemble_combine: {len(xs)} members (1..{L.ENSEMBLE_MAX})")
    if w.dtype != torch.float32 or w.numel() < L.ENSEMBLE_MAX or out.dtype != torch.float32:
        raise TypeError("ensemble_combine: w is fp32 [8] and out fp32")
    d = L.EnsembleDesc()
    d.n, d.mode, d.rows, d.V = len(xs), L.ENS_MODE[mode], out.shape[0], int(cols or out.shape[1])
    for m, x in enumerate(xs):
        if x.shape[0] != out.shape[0]:
            raise ValueError("ensemble_combine: every member has out's rows")
        d.dtype[m], d.x[m], d.ld[m] = L.dtype_code(x.dtype), x.data_ptr(), _ld(x)
    d.w, d.out, d.ld_out = w.data_ptr(), out.data_ptr(), _ld(out)
    L.check(L.load().vct_ensemble_combine(L.C.byref(d), L.stream_ptr()), "vct_ensemble_combine")
    return out


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
