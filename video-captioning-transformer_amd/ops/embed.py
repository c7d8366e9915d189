"""Token embedding forward / backward with its live-row table, and the text tower's pooled output."""
import torch

from .. import _lib as L
from ._common import Drop, _drop


def embed_fwd(ids, S, table, pos, x, dropout: Drop = None):
    """ids: int64 [B, S_total] (row stride = ids.stride(0)); uses the first S columns of each row."""
    B = ids.shape[0]
    s, site, p = _drop(dropout)
    L.check(L.load().vct_embed_fwd(L.dtype_code(x.dtype), B, S, x.shape[1], ids.data_ptr(), ids.stride(0),
                                   table.data_ptr(), pos.data_ptr(), x.data_ptr(), s, site, p, L.stream_ptr()),
            "vct_embed_fwd")
    return x


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
