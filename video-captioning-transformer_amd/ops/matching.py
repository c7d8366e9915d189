"""The video-text matching task (csrc/vct_match.hip) and retrieval evaluation over a whole split (csrc/vct_retrieval.hip)."""
import torch

from .. import _lib as L
from ._common import _ld


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
