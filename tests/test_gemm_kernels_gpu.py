"""Kernel-level tests (GPU) of the GEMM family -- vct_gemm, vct_gemm_grouped -- through ops.gemm / ops.gemm_grouped only, every element
against the fp64 reference of the same operation (tests/gemm_ref.py, itself checked by tests/test_gemm_ref_cpu.py, which also shows that
each checker used here rejects a dropped K element, a dropped K tile of one 16 x 16 block, swapped rows, shifted columns, a shifted
bias, a partial summed twice and a truncated bf16 result).

Harness.  Outputs (C, preact, bias_grad, the Adam tensors) live in an Arena filled with 0xFF, 64 canary bytes on both sides of each;
they are strided views (ldc > N) wherever the route allows it and the padding columns must stay 0xFF.  Operands carry NaN everywhere a
kernel must not read, or whose value must not reach a valid output: rows behind M / N / K, columns behind k_valid and n_valid (and, for
the M-contiguous operands, behind m_valid) inside the leading dimension, bias elements behind N; split-K workspaces are NaN on entry.
Every call runs twice on fresh arenas: the two arenas must be byte-identical, every valid output finite, every canary intact; a
GemmScratch's counters are all zero afterwards.  Every case asserts ops.gemm_last_route() against the route it was written for: when
an eligibility threshold moves, the case FAILS instead of silently testing another kernel.

Checks.  Integer operands in [-3, 3] (gemm_ref.ints): exact in any summation order, any split, on any MFMA -- fp32 output, bf16
output (one RNE rounding), the saved pre-activation and the bias gradient must equal the reference bit for bit (with ReLU, ReLU', integer
bias and addend too).  GELU, GELU' and dropout (1 / (1 - p) is no integer) are judged against the per-element bounds of gemm_ref.bound on
integer AND random operands, the dropout mask exactly (gemm_ref.check_mask).  No bound is sized from the kernels under test.

The shapes are the smallest at which each kernel can still go wrong (gemm_ref.TILES ...), not the workload's; one pytest case per kernel
variant, layout and output type, the shapes looped inside."""
import math

import pytest
import torch

import gemm_ref as G
from gpu_arena import Arena, up

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
NAN = float("nan")
LAYOUT = {"NT": (False, True), "NN": (False, False), "TN": (True, False)}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from vct_amd import ops as _ops
    return _ops


_VALS = {}


def values(kind, rows, cols, seed, dtype, scale=1.0):
    """Operand values on the device, generated once per (kind, shape, seed, type)."""
    key = (kind, rows, cols, seed, dtype, scale)
    if key not in _VALS:
        _VALS[key] = G.ints((rows, cols), seed, dtype, DEV) if kind == "ints" else G.rnd((rows, cols), seed, scale, dtype, DEV)
    return _VALS[key]


def poison(vals, width=None, extra=2):
    """The [R, width or C] view of a NaN buffer [R + extra, ld] that holds vals in its first C columns: NaN in the rows behind R, in
    the view's columns behind C (k_valid / n_valid / m_valid inside the view) and in the leading dimension's padding."""
    R, C = vals.shape
    q = 16 // vals.element_size()
    W = C if width is None else width
    buf = torch.full((R + extra, up(W, q) + q), NAN, dtype=vals.dtype, device=DEV)
    buf[:R, :C] = vals
    return buf[:R, :W]


_SCRATCH = {}


def scratch(ops):
    if "s" not in _SCRATCH:
        _SCRATCH["s"] = ops.GemmScratch(DEV)
    s = _SCRATCH["s"]
    s.ws.fill_(NAN)
    return s


_REF = {}
ASSERTED_KERNELS = set()          # kernel ids whose route assertion passed in this session


def reference(key, a, b, ta, tb, M, N, K):
    """(Z, S) in fp64 on the device, computed once per operand set."""
    if key not in _REF:
        _REF[key] = G.product(a, b, ta, tb, M, N, K)
    return _REF[key]


# ---- one case: build, run twice, compare ----------------------------------------------------------------------------------------------------
def run(ops, layout, M, N, K, *, out=BF, dt=BF, kind="ints", tile=0, split_k=0, ws=None, bias=False, act=None, preact=False, addend=False,
        dact=False, drop=None, bias_grad=False, ldc=None, skew=0, ld_add=None, ld_pre=None, skew_pre=0, adam=False, route=None, seed=1, what=None,
        keep_ref=True):
    ta, tb = LAYOUT[layout]
    what = what or f"{layout} {M}x{N}x{K} {'bf16' if out == BF else 'fp32'} tile {tile}"
    q = 16 // torch.empty(0, dtype=dt).element_size()
    sc = 1.0 / math.sqrt(K)
    # operands: K-contiguous ones are [rows, K] views of width up(K, q) (NaN behind k_valid), the others [K, rows] with NaN behind the rows
    av = values(kind, K, M, seed, dt) if ta else values(kind, M, K, seed, dt)
    bv = values(kind, N, K, seed + 1, dt, sc) if tb else values(kind, K, N, seed + 1, dt, sc)
    a = poison(av, None if ta else up(K, q))
    b = poison(bv, up(K, q) if tb else None)
    kw = dict(ta=ta, tb=tb, m_valid=M, n_valid=N, k_valid=K, tile=tile, split_k=split_k)
    ekw = {}
    if bias:
        bias_v = values(kind, 1, N, seed + 2, F32, 0.5)
        kw["bias"] = poison(bias_v, extra=0)[0]
        ekw["bias"] = bias_v[0]
    ld_o = up(N, 8) + 8 if ldc is None else ldc
    ld_x = ld_o if ld_add is None else ld_add
    for name, on, s in (("addend", addend, 3), ("dact_src", dact, 4)):
        if on:
            v = values(kind, M, N, seed + s, out)
            buf = torch.full((M + 2, ld_x), NAN, dtype=out, device=DEV)
            buf[:M, :N] = v
            kw[name] = buf[:M, :N]
            ekw[name] = v
    if act is not None:
        kw["act"] = ekw["act"] = act
    seed_t = None
    if drop is not None:
        seed_t = torch.tensor([drop[0]], dtype=torch.int32, device=DEV)
        kw["dropout"] = (seed_t, drop[1], drop[2])
        ekw["drop"] = drop
    specs = [("C", M, N, out, ld_o, skew)]
    if preact:
        specs.append(("preact", M, N, out, ld_o if ld_pre is None else ld_pre, skew_pre))
    if bias_grad:
        specs.append(("bias_grad", 1, M, F32, M, 0))
    if adam:
        specs += [(n, M, N, F32, ld_o, 0) for n in ("param", "exp_avg", "exp_avg_sq")]
    arenas, routes = [], []
    for rep in range(2):
        ar = Arena(specs)
        if ws == "plain":
            kw["workspace"] = torch.full(((64 if M * N < (1 << 19) else 16) * (M * N + M) + 64,), NAN, dtype=F32, device=DEV)
        elif ws == "scratch":
            kw["workspace"] = scratch(ops)
        if preact:
            kw["preact"] = ar["preact"]
        if bias_grad:
            kw["bias_grad"] = ar["bias_grad"][0]
        keep = None
        if adam:
            from vct_amd import _lib as L
            ar["param"].copy_(values("rnd", M, N, seed + 7, F32)); ar["exp_avg"].copy_(values("rnd", M, N, seed + 8, F32, 0.01))
            ar["exp_avg_sq"].copy_(values("rnd", M, N, seed + 9, F32, 0.01) ** 2)
            step = torch.tensor([2], dtype=torch.int32, device=DEV)
            hyper = torch.tensor([1e-3, 0.9, 0.999, 1e-8, 0.01, 0, 0, 0], dtype=F32, device=DEV)
            ad = L.GemmAdam()
            ad.param, ad.exp_avg, ad.exp_avg_sq = ar["param"].data_ptr(), ar["exp_avg"].data_ptr(), ar["exp_avg_sq"].data_ptr()
            ad.hyper, ad.step, ad.store_grad = hyper.data_ptr(), step.data_ptr(), 1
            kw["adam"] = ad
            keep = (step, hyper, ad)
        ops.gemm(a, b, ar["C"], **kw)
        routes.append(ops.gemm_last_route())
        torch.cuda.synchronize()
        ar.check()
        if ws == "scratch":
            assert int(kw["workspace"].counters.abs().sum()) == 0, f"{what}: tile counters not zero after the call"
        arenas.append(ar)
        del keep
    assert routes[0] == routes[1], (what, routes)
    assert torch.equal(arenas[0].buf, arenas[1].buf), f"{what}: the second call's outputs differ from the first's"
    r = routes[0]
    if route is not None:
        got = {k: r[k] for k in route}
        assert got == route, f"{what}: took route {r}, written for {route}"
        if "kernel" in route:
            ASSERTED_KERNELS.add(r["kernel"])
    ar = arenas[0]
    # reference
    rkey = (layout, M, N, K, dt, kind, seed)
    Z, S = reference(rkey, a, b, ta, tb, M, N, K) if keep_ref else G.product(a, b, ta, tb, M, N, K)
    e = G.epilogue(Z, **ekw)
    exact = kind == "ints"
    worst = 0.0
    if exact and act != "gelu" and drop is None:
        G.check_exact(what, ar["C"], e["out"])
    else:
        worst = G.check_elem(what, ar["C"], e["out"], G.bound(e["out"], S, K, out, ekw.get("bias"), act, e))
    if drop is not None and not addend:
        G.check_mask(what + " mask", ar["C"], e["out"], G.gelu_tiny(e["z"]) if (act == "gelu" and not dact) else None)
    if preact:
        if exact:
            G.check_exact(what + " preact", ar["preact"], e["preact"])
        else:
            G.check_elem(what + " preact", ar["preact"], e["preact"], G.bound(e["preact"], S, K, out, ekw.get("bias"), what="preact"))
    if bias_grad:
        bg = G.bias_grad(a, ta, M, K)
        if exact:
            G.check_exact(what + " bias_grad", ar["bias_grad"][0], bg)
        else:
            sa = G.bias_grad(a.abs(), ta, M, K)
            G.check_elem(what + " bias_grad", ar["bias_grad"][0], bg, G.U24 * bg.abs() + (K + 1) * G.U24 * sa)
    return dict(C=ar["C"], route=r, arena=ar, worst=worst)


def shapes_for(code):
    bm, bn = G.TILES[code]
    return G.general_mn(bm, bn)


def general_route(code, nbuf, split=1):
    bm, bn = G.TILES[code]
    return dict(kernel=1, bm=bm, bn=bn, nbuf=nbuf, variant=G.VARIANT[code], split=split)


# ---- general bf16 kernel, forced through the tile override --------------------------------------------------------------------------------
GENERAL = [(c, nb, lay, o) for c in (1, 2, 3, 4, 5, 8) for nb in (1, 2) for lay in ("NT", "NN", "TN") for o in (BF, F32)] + \
          [(c, 2, lay, BF) for c in (6, 7, 9) for lay in ("NT", "NN")]


@pytest.mark.parametrize("code,nbuf,layout,out", GENERAL, ids=lambda v: {BF: "bf16", F32: "fp32"}.get(v, str(v)))
def test_general_kernel_every_tile_layout_and_output_type(ops, code, nbuf, layout, out):
    """Tile `code` with `nbuf` operand stages (tile + 10 * nbuf); (M, N) around the tile's edges; K = 8 (the tail path only), 64, 72,
    192 (the two-stage ring wraps), 200, 203 (through k_valid: a tail that is no multiple of 8); vector stores with a ragged last
    chunk (ldc a multiple of 8), and the scalar path: N = 77 with ldc = 77, and a C that starts one element into its buffer."""
    tile = code + 10 * nbuf if code not in (6, 7, 9) else code
    route = general_route(code, nbuf)
    bm, bn = G.TILES[code]
    for K in G.GENERAL_K:
        for M, N in shapes_for(code):
            run(ops, layout, M, N, K, out=out, tile=tile, route=route, bias_grad=(layout == "TN" and out == F32))
        run(ops, layout, bm + 1, 77, K, out=out, tile=tile, route=route, ldc=77)
    run(ops, layout, bm + 1, bn - 1, 203, out=out, tile=tile, route=route, skew=1, ldc=bn + 7)


EPI = {
    "bias": dict(bias=True),
    "bias_gelu_preact": dict(bias=True, act="gelu", preact=True),
    "relu": dict(act="relu"),
    "addend": dict(addend=True),
    "dgelu": dict(act="gelu", dact=True),
    "drelu": dict(act="relu", dact=True),
    "dropout": dict(drop=(77, 9, 0.3)),
    "bias_gelu_dropout": dict(bias=True, act="gelu", drop=(81, 7, 0.3)),
    "dgelu_dropout": dict(act="gelu", dact=True, drop=(78, 4, 0.3)),
    "forward_all": dict(bias=True, act="gelu", preact=True, drop=(79, 5, 0.3), addend=True),
    "forward_all_relu": dict(bias=True, act="relu", preact=True, addend=True),
    "derivative_all": dict(bias=True, act="relu", dact=True, drop=(80, 6, 0.3), addend=True),
}
WORST = {}


def _epi_runs(ops, layout, M, N, K, epi, **kw):
    """The integer run always; GELU, a derivative or dropout also on random operands."""
    r = run(ops, layout, M, N, K, **EPI[epi], **kw)
    w = r["worst"]
    e = EPI[epi]
    if e.get("act") == "gelu" or e.get("dact") or e.get("drop"):
        w = max(w, run(ops, layout, M, N, K, kind="rnd", seed=11, **e, **kw)["worst"])
    WORST[epi] = max(WORST.get(epi, 0.0), w)


@pytest.mark.parametrize("out", [BF, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("epi", list(EPI))
@pytest.mark.parametrize("code", [4, 5])
def test_general_kernel_epilogues(ops, code, epi, out):
    """Forward epilogues on the NT form, derivative ones on the NN form (dX = dY W times act'), both store paths."""
    layout = "NN" if EPI[epi].get("dact") else "NT"
    route = general_route(code, 2)
    bm, bn = G.TILES[code]
    for K in (8, 72, 203):
        for M, N in shapes_for(code) + ((bm + 1, 77),):
            _epi_runs(ops, layout, M, N, K, epi, out=out, tile=code, route=route, ldc=77 if N == 77 else None, ld_add=80 if N == 77 else None)
    print(f"[gemm] epilogue {epi}: worst |delta| / bound = {WORST[epi]:.3f}")


# ---- split-K on the general kernel ------------------------------------------------------------------------------------------------------------
# nkt = 16 (K = 1000, one ragged tile) / 17 (K = 1032); forced split -> (K tiles per split, splits): a short last split and the clamp
# to nkt / 2, worked out by hand from the header's rule "split <= nkt / 2, then ceil(nkt / ceil(nkt / split))"
SPLITS = {(16, 2): 2, (16, 5): 4, (16, 8): 8, (17, 2): 2, (17, 5): 5, (17, 8): 6, (16, 0): 8, (17, 0): 6}


@pytest.mark.parametrize("out", [BF, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("code", [4, 5])
@pytest.mark.parametrize("layout", ["NT", "NN", "TN"])
def test_general_kernel_split_k_two_pass_and_single_pass(ops, layout, code, out):
    """Forced splits 2, 5, 8 and the automatic one; the two-pass reduce (plain workspace: a reduce launch follows) and the single-pass
    reduce (GemmScratch: tile counters, no second launch) give the same bits; TN with fp32 output carries the bias gradient through
    the partial rows."""
    bg = layout == "TN" and out == F32
    for K in G.SPLIT_K:
        nkt = (K + 63) // 64
        for M, N, ldc in ((130, 72, None), (65, 77, 77)):
            for sk in (2, 5, 8, 0):
                split = SPLITS[(nkt, sk)]
                two = run(ops, layout, M, N, K, out=out, tile=code, split_k=sk, ws="plain", bias_grad=bg, ldc=ldc,
                          route=dict(general_route(code, 2, split), in_kernel_reduce=False, reduce_launch=True))
                one = run(ops, layout, M, N, K, out=out, tile=code, split_k=sk, ws="scratch", bias_grad=bg, ldc=ldc,
                          route=dict(general_route(code, 2, split), in_kernel_reduce=True, reduce_launch=False))
                assert torch.equal(two["arena"].buf, one["arena"].buf), f"{layout} {M}x{N}x{K} split {sk}: the two reduces differ"


@pytest.mark.parametrize("out", [BF, F32], ids=["bf16", "fp32"])
def test_general_kernel_split_k_with_an_epilogue(ops, out):
    """A GEMM with an epilogue splits only with tile counters (the last workgroup of a tile applies the epilogue to the summed
    partials) and, on its own, only for M <= 16."""
    for K in G.SPLIT_K:
        nkt = (K + 63) // 64
        for M in (1, 7, 16):
            for epi in ("bias_gelu_preact", "forward_all_relu", "forward_all"):
                _epi_runs(ops, "NT", M, 72, K, epi, out=out, tile=4, ws="scratch",
                          route=dict(general_route(4, 2, SPLITS[(nkt, 0)]), in_kernel_reduce=True, reduce_launch=False))
            _epi_runs(ops, "NN", M, 72, K, "dgelu_dropout", out=out, tile=4, ws="scratch", split_k=5,
                      route=dict(general_route(4, 2, SPLITS[(nkt, 5)]), in_kernel_reduce=True, reduce_launch=False))
        # M > 16: no automatic split with an epilogue; without counters none at all
        _epi_runs(ops, "NT", 17, 72, K, "bias", out=out, tile=4, ws="scratch", route=general_route(4, 2, 1))
        _epi_runs(ops, "NT", 16, 72, K, "bias", out=out, tile=4, ws="plain", route=general_route(4, 2, 1))


def test_general_kernel_single_pass_reduce_is_refused_above_16_mb_of_partials(ops):
    """8 x 1024 x 1024 fp32 partials = 32 MB: with tile counters on offer the plain product falls back to the two-pass reduce; 4 splits
    (16 MB) still reduce in the kernel.  A product with an epilogue cannot take the two-pass reduce: its FORCED split of 8 is refused
    with VCT_E_WORKSPACE (like a forced split without a workspace), its automatic split is none."""
    M = N = 1024
    K = 1000
    run(ops, "NT", M, N, K, tile=5, split_k=8, ws="scratch", route=dict(general_route(5, 2, 8), in_kernel_reduce=False, reduce_launch=True))
    run(ops, "NT", M, N, K, tile=5, split_k=5, ws="scratch", route=dict(general_route(5, 2, 4), in_kernel_reduce=True, reduce_launch=False))
    run(ops, "NT", M, N, K, tile=5, ws="scratch", bias=True, route=dict(general_route(5, 2, 1), in_kernel_reduce=False, reduce_launch=False))
    a, b = values("ints", M, K, 1, BF), values("ints", N, K, 2, BF)
    with pytest.raises(ValueError, match="VCT_E_WORKSPACE"):
        ops.gemm(a, b, torch.empty(M, N, dtype=BF, device=DEV), bias=values("ints", 1, N, 3, F32)[0], tile=5, split_k=8, workspace=scratch(ops))


# ---- fp32 (parity-mode) kernel ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["NT", "NN", "TN"])
def test_fp32_kernel_both_tiles(ops, layout):
    """dtype fp32: the 64 x 64 tile at small shapes, the 128 x 128 tile from 384 tiles of 128 x 128 on (2049 x 3080: 17 x 25 ragged
    tiles); K = 4 and 20 (a ragged 16-deep tile), 16, 52; integers exactly, random operands against the fp32 bound."""
    for K in G.F32_K:
        for M, N in G.general_mn(64, 64):
            for kind in ("ints", "rnd"):
                run(ops, layout, M, N, K, out=F32, dt=F32, kind=kind, bias=(kind == "rnd"), bias_grad=(layout == "TN"),
                    route=dict(kernel=2, bm=64, bn=64, split=1))
        run(ops, layout, 65, 77, K, out=F32, dt=F32, ldc=77, skew=1, route=dict(kernel=2, bm=64, bn=64, split=1))
    for K in G.F32_K:
        for kind in ("ints", "rnd"):
            run(ops, layout, 2049, 3080, K, out=F32, dt=F32, kind=kind, bias=(kind == "rnd"), bias_grad=(layout == "TN"),
                route=dict(kernel=2, bm=128, bn=128, split=1), keep_ref=False)


@pytest.mark.parametrize("epi", ["bias_gelu_preact", "forward_all", "derivative_all", "dgelu"])
def test_fp32_kernel_epilogues(ops, epi):
    layout = "NN" if EPI[epi].get("dact") else "NT"
    for M, N, K in ((65, 63, 20), (63, 65, 52), (131, 8, 16)):
        _epi_runs(ops, layout, M, N, K, epi, out=F32, dt=F32, route=dict(kernel=2, bm=64, bn=64))


# ---- skinny kernel --------------------------------------------------------------------------------------------------------------------------------
def skinny_ntl(M, N):
    """The three column-tile counts, as the shapes of this file select them (csrc/vct_gemm_skinny.hip, skinny_ntl: the widest of
    4 / 2 / 1 that leaves 192 workgroups): 16 row tiles x 256 column tiles -> 4; 2 x 256 -> 2; everything else here -> 1."""
    return 4 if (M, N) == (256, 4096) else (2 if (M, N) == (17, 4096) else 1)


@pytest.mark.parametrize("out", [BF, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("epi", [None, "bias", "bias_gelu", "relu", "addend"])
def test_skinny_kernel_all_three_widths(ops, epi, out):
    e = dict(bias=True, act="gelu") if epi == "bias_gelu" else (EPI[epi] if epi else {})
    for K in G.SKINNY_K:
        for N in G.SKINNY_N:
            for M in G.SKINNY_M:
                ntl = skinny_ntl(M, N)
                route = dict(kernel=3, bm=16, bn=16 * ntl, variant=ntl, split=1)
                run(ops, "NT", M, N, K, out=out, route=route, **e)
                if epi == "bias_gelu" and (K, N) in ((72, 17), (8192, 4096)):
                    run(ops, "NT", M, N, K, out=out, kind="rnd", seed=11, route=route, **e)


def test_skinny_kernel_limits_route_to_the_general_kernel(ops):
    """Just outside each limit of the skinny kernel the route names the general kernel (and the result is still exact); with a saved
    pre-activation or dropout too."""
    for M, N, K in ((257, 64, 64), (16, 15, 64), (16, 64, 56), (16, 64, 76), (256, 4104, 64), (16, 64, 8200)):
        run(ops, "NT", M, N, K, bias=True, route=dict(kernel=1))
    run(ops, "NT", 16, 64, 64, bias=True, act="relu", preact=True, route=dict(kernel=1))
    run(ops, "NT", 16, 64, 64, drop=(5, 1, 0.3), route=dict(kernel=1))
    run(ops, "NT", 16, 64, 64, dt=F32, out=F32, route=dict(kernel=2))
    run(ops, "NN", 16, 64, 64, route=dict(kernel=1))
    run(ops, "NT", 256, 4096, 8192, bias=True, route=dict(kernel=3, bn=64))


# ---- persistent-tile layer kernel -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("epi", [None, "bias", "forward_all_relu", "forward_all", "dgelu_dropout", "derivative_all"])
@pytest.mark.parametrize("mode", ["auto", "forced"])
@pytest.mark.parametrize("layout", ["NT", "NN"])
def test_layer_kernel_both_tile_heights(ops, layout, mode, epi):
    """128 x 128 tiles at N >= 1024 (taken without an override: NT only; NN through tile=100), 64 x 128 tiles forced with tile=100 at
    N = 256; the plain instantiation (nothing / bias) and the epilogue one."""
    N, bm = (1032, 128) if mode == "auto" else (256, 64)
    tile = 0 if (mode == "auto" and layout == "NT") else 100
    variant = 0 if epi in (None, "bias") else 1
    route = dict(kernel=6, bm=bm, bn=128, variant=variant, split=1)
    for K in G.PT_K:
        for M in G.PT_M:
            if epi is None:
                run(ops, layout, M, N, K, tile=tile, route=route)
            else:
                _epi_runs(ops, layout, M, N, K, epi, tile=tile, route=route)


def test_layer_kernel_routes_away(ops):
    """tile=99 forbids the kernel; a misaligned preact / addend / dact_src, a C whose leading dimension is no multiple of 8, an NN
    product without the override and shapes outside its limits go to the general kernel instead of failing."""
    M, N, K = 1025, 1032, 136
    run(ops, "NT", M, N, K, bias=True, route=dict(kernel=6, bm=128))
    run(ops, "NT", M, N, K, bias=True, tile=99, route=dict(kernel=1))
    run(ops, "NT", M, N, K, act="relu", addend=True, ld_add=N + 4, route=dict(kernel=1))
    run(ops, "NN", M, N, K, act="relu", dact=True, ld_add=N + 4, tile=100, route=dict(kernel=1))
    run(ops, "NT", M, N, K, bias=True, act="relu", preact=True, route=dict(kernel=6, bm=128, variant=1))      # aligned preact: taken
    run(ops, "NT", M, N, K, bias=True, act="relu", preact=True, ld_pre=N + 4, route=dict(kernel=1))           # aligned C, preact ld N + 4
    run(ops, "NT", M, N, K, bias=True, act="relu", preact=True, ld_pre=N + 4, skew_pre=1, tile=100, route=dict(kernel=1))   # ... one element in
    run(ops, "NT", M, N, K, bias=True, ldc=N + 4, route=dict(kernel=1))
    run(ops, "NT", M, N, K, bias=True, skew=1, ldc=N + 8, tile=100, route=dict(kernel=1))
    run(ops, "NN", M, N, K, route=dict(kernel=1))
    run(ops, "NT", 1023, N, K, route=dict(kernel=1))
    run(ops, "NT", M, 1016, K, route=dict(kernel=1))
    run(ops, "NT", M, N, 120, route=dict(kernel=1))
    run(ops, "NT", M, 248, K, tile=100, route=dict(kernel=1))
    run(ops, "NT", M, N, K, out=F32, route=dict(kernel=1))


# ---- persistent 256 x 256 kernels: one case per branch of gemm256_try ---------------------------------------------------------------------------------
@pytest.mark.parametrize("bias", [False, True], ids=["plain", "bias"])
def test_g256_nt_forward(ops, bias):
    M, N, K = G.G256["nt"]
    for kind in ("ints", "rnd"):
        run(ops, "NT", M, N, K, bias=bias, kind=kind, route=dict(kernel=4, bm=256, bn=256, split=1, reduce_launch=False), keep_ref=False)


def test_g256_nt_split_over_k(ops):
    M, N, K = G.G256["nt_splitk"]
    for kind in ("ints", "rnd"):
        r = run(ops, "NT", M, N, K, kind=kind, ws="plain", route=dict(kernel=4, bm=256, bn=256, in_kernel_reduce=False, reduce_launch=True),
                keep_ref=False)
        assert r["route"]["split"] >= 2


def test_g256_nn_on_the_pipelined_kernel_and_its_fallback(ops):
    """NN over a vocabulary-long K: 4 tiles -> 64 splits asked, 129 K stages -> 3 per split, 43 splits, every one with two full
    stages: the pipelined kernel.  A forced split of 40 gives 4 stages per split and leaves stage 128 (the ragged one) alone in split
    33: g32_eligible fails and the round-5 kernel takes the product."""
    M, N, K = G.G256["nn"]
    for kind in ("ints", "rnd"):
        run(ops, "NN", M, N, K, kind=kind, ws="plain", route=dict(kernel=5, bm=256, bn=256, split=43, reduce_launch=True))
        run(ops, "NN", M, N, K, kind=kind, ws="plain", split_k=40, route=dict(kernel=4, bm=256, bn=256, split=33, reduce_launch=True))


def test_g256_tn_weight_gradient_and_the_optimizer_epilogue(ops):
    """TN, 16 x 13 = 208 tiles, 33 K stages (the last one ragged), bias gradient; with a GemmAdam that keeps the gradient
    (store_grad = 1) C is bit-identical to the call without the optimizer (tests/test_kernels_gpu.py keeps the parameter arithmetic)."""
    M, N, K = G.G256["tn"]
    route = dict(kernel=5, bm=256, bn=256, split=1, reduce_launch=False)
    plain = run(ops, "TN", M, N, K, out=F32, bias_grad=True, route=route, keep_ref=False)
    fused = run(ops, "TN", M, N, K, out=F32, bias_grad=True, adam=True, route=route, keep_ref=False)
    assert torch.equal(plain["C"], fused["C"])
    run(ops, "TN", M, N, K, out=F32, bias_grad=True, kind="rnd", route=route, keep_ref=False)


# ---- grouped launch -----------------------------------------------------------------------------------------------------------------------------------
GROUP_ODD, GROUP_ODD_ROWS = 5, 584        # problem 5 reduces over its own row count: the per-problem splits differ


def group_rows(rows):
    return [GROUP_ODD_ROWS if i == GROUP_ODD else rows for i in range(len(G.GROUP_MN))]


def group_splits(rows, tile, split_k):
    """The documented plan of vct_gemm_grouped: one tile for the group; split 1 from 192 tiles on, else ceil(256 / tiles); a forced
    split_k instead; per problem never more than nkt / 4; then ceil(nkt / ceil(nkt / split))."""
    bm, bn = G.TILES[tile]
    gt = sum(((m + bm - 1) // bm) * ((n + bn - 1) // bn) for m, n in G.GROUP_MN)
    out = []
    for k in group_rows(rows):
        nkt = (k + 63) // 64
        s = split_k if split_k >= 1 else (1 if gt >= 192 else (255 + gt) // gt)
        s = max(1, min(s, max(nkt // 4, 1)))
        per = (nkt + s - 1) // s
        out.append((nkt + per - 1) // per)
    return out


@pytest.mark.parametrize("split_k", [0, 3], ids=["auto", "split3"])
@pytest.mark.parametrize("tile", [5, 8, 4])
def test_grouped_weight_gradients(ops, tile, split_k):
    """Eight problems of different shapes (200 x 72 and 1 x 8 among them) over 8, 328, 1000 and 1003 rows (one of them over 584), one without a bias
    gradient, every dW / db a view into ONE flat arena tensor; every dW and db exact."""
    bm, bn = G.TILES[tile]
    NO_DB = 2
    for rows in G.GROUP_ROWS:
        ks = group_rows(rows)
        dys = [poison(values("ints", ks[i], m, 20 + i, BF)) for i, (m, n) in enumerate(G.GROUP_MN)]
        xs = [poison(values("ints", ks[i], n, 40 + i, BF)) for i, (m, n) in enumerate(G.GROUP_MN)]
        tot = sum(m * n for m, n in G.GROUP_MN)
        totb = sum(m for i, (m, n) in enumerate(G.GROUP_MN) if i != NO_DB)
        arenas, routes = [], []
        for rep in range(2):
            ar = Arena([("dW", 1, tot, F32, tot, 0), ("db", 1, totb, F32, totb, 0)])
            items, at, bt = [], 0, 0
            for i, (m, n) in enumerate(G.GROUP_MN):
                dw = ar["dW"][0, at:at + m * n].view(m, n)
                at += m * n
                db = None
                if i != NO_DB:
                    db = ar["db"][0, bt:bt + m]
                    bt += m
                items.append((dys[i], xs[i], dw, db))
            sc = scratch(ops)
            ops.gemm_grouped(items, sc, split_k=split_k, tile=tile)
            routes.append(ops.gemm_last_route())
            torch.cuda.synchronize()
            ar.check()
            assert int(sc.counters.abs().sum()) == 0, "tile counters not zero after the launch"
            arenas.append((ar, items))
        r = routes[0]
        assert routes[0] == routes[1]
        assert r["kernel"] == 7 and (r["bm"], r["bn"], r["variant"]) == (bm, bn, G.VARIANT[tile]), r
        ASSERTED_KERNELS.add(7)
        assert r["group_splits"] == group_splits(rows, tile, split_k), (r, rows)
        assert rows != 1000 or len(set(r["group_splits"])) > 1             # (the odd problem's entry is its own)
        assert r["split"] == max(r["group_splits"]) and r["in_kernel_reduce"] == (r["split"] > 1) and not r["reduce_launch"]
        assert torch.equal(arenas[0][0].buf, arenas[1][0].buf), f"grouped rows {rows}: the second launch differs from the first"
        for i, (dy, x, dw, db) in enumerate(arenas[0][1]):
            m, n = G.GROUP_MN[i]
            Z, _ = G.product(dy, x, True, False, m, n, ks[i])
            G.check_exact(f"grouped tile {tile} rows {rows} dW[{i}] {m}x{n}", dw, Z)
            if db is not None:
                G.check_exact(f"grouped tile {tile} rows {rows} db[{i}]", db, G.bias_grad(dy, True, m, ks[i]))


# ---- coverage of the declared routes ------------------------------------------------------------------------------------------------------------------
def test_case_tables_cover_every_tile_code_layout_and_width():
    """The case tables name every tile code of the general kernel with both stage counts, every layout x output type, and all three
    widths of the skinny kernel (this test reads the tables, it needs no device work)."""
    assert {c for c, _, _, _ in GENERAL} == {1, 2, 3, 4, 5, 6, 7, 8, 9}
    assert {(c, nb) for c, nb, _, _ in GENERAL} >= {(c, nb) for c in (1, 2, 3, 4, 5, 8) for nb in (1, 2)}
    assert {(lay, o) for c, _, lay, o in GENERAL if c in (1, 2, 3, 4, 5, 8)} == {(lay, o) for lay in LAYOUT for o in (BF, F32)}
    assert {skinny_ntl(m, n) for m in G.SKINNY_M for n in G.SKINNY_N} == {1, 2, 4}


def test_route_assertions_reached_every_kernel_id():
    """Runs after the cases of this file (select it together with them): the route assertions that passed in this session name
    every kernel id -- 1 general bf16, 2 general fp32, 3 skinny, 4 / 5 persistent 256 (round-5 / pipelined), 6 layer kernel, 7 grouped."""
    assert ASSERTED_KERNELS == {1, 2, 3, 4, 5, 6, 7}, ASSERTED_KERNELS
