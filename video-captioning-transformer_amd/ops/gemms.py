"""The GEMM family (csrc/vct_gemm*.hip): single, grouped weight-gradient, route record, workspace bound."""
from typing import Optional

import torch

from .. import _lib as L
from ._common import Drop, _drop, _ld
from .runtime import TAPS, tap, tap_active


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
    tag: a key of TAPS -- the launch is bracketed with timing events while that tap is active (runtime.taps_enable).
    adam: L.GemmAdam (weight-gradient form only) -- torch.optim.Adam's step on the matrix runs in the epilogue (include/vct_hip.h)."""
    lib = L.load()
    d = _gemm_desc(a, b, out, ta, tb, bias, act, preact, addend, dact_src, dropout, bias_grad, workspace, split_k,
                   n_valid, k_valid, m_valid, adam)
    d.reserved = tile       # kernel selection override (include/vct_hip.h, vct_gemm_desc.reserved): tests and A/B probes
    timed = tag in TAPS and tap_active(tag)
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
