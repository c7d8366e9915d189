"""CPU checks of tests/gemm_ref.py, the fp64 reference and the checkers of tests/test_gemm_kernels_gpu.py (no GPU, no library):
  * epilogue() against torch.nn.functional.linear / gelu / relu and, for the derivative form, against autograd;
  * a CORRECT emulation of the kernels' arithmetic (bf16 operands, fp32 accumulation in K tiles of 64, split partials summed in a
    shuffled order, one rounding of the result) stays inside the bounds at every shape the GPU file runs, and is bit-exact on the
    integer inputs;
  * every seeded fault applied to that emulation is rejected by the checker the GPU file uses for it -- the evidence that the GPU
    tests would fail on a subtly wrong kernel.
At shapes with more than 64 rows / columns the emulation runs on the first 64 (rows and columns of a product are independent, and the
bound of an element depends on K and its own operands only: K is never cut)."""
import math

import pytest
import torch

import gemm_ref as G

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64


def _operands(M, N, K, seed, exact, dtype=BF):
    M, N = min(M, 64), min(N, 64)                          # (see the module docstring)
    if exact:
        return G.ints((M, K), seed, dtype), G.ints((N, K), seed + 1, dtype), G.ints((N,), seed + 2)
    return G.rnd((M, K), seed, 1.0, dtype), G.rnd((N, K), seed + 1, 1.0 / math.sqrt(K), dtype), G.rnd((N,), seed + 2, 0.5)


def test_epilogue_is_linear_activation_dropout_addend():
    a, w, b = G.rnd((37, 72), 1).double(), G.rnd((29, 72), 2).double(), G.rnd((29,), 3).double()
    add = G.rnd((37, 29), 4).double()
    Z, S = G.product(a, w)
    assert torch.allclose(S, a.abs() @ w.abs().t(), rtol=1e-13)
    lin = torch.nn.functional.linear(a, w, b)
    for act, fn in (("gelu", torch.nn.functional.gelu), ("relu", torch.relu), (None, lambda x: x)):
        e = G.epilogue(Z, bias=b, act=act, addend=add)
        assert torch.allclose(e["preact"], lin, rtol=1e-13, atol=1e-13)
        assert torch.allclose(e["out"], fn(lin) + add, rtol=1e-12, atol=1e-13)
    # dropout: on C, BEFORE the addend; idx = row * N + col; the multiplier is 0 or 1 / (1 - p) in fp32
    drop = (77, 9, 0.3)
    e = G.epilogue(Z, bias=b, act="relu", addend=add, drop=drop)
    m = e["mask"]
    assert set(m.unique().tolist()) == {0.0, float(torch.tensor(1.0, dtype=F32) / (1 - torch.tensor(0.3, dtype=F32)))}
    assert 0.6 < float((m != 0).double().mean()) < 0.8
    assert torch.equal(e["out"], torch.relu(lin) * m + add)
    assert torch.equal(e["out"][m == 0], add[m == 0])                       # a dropped element still receives the addend
    assert torch.equal(G.drop_mask(37, 29, drop)[5, 7], torch.from_numpy(G.LR.drop_mult(77, 9, 0.3, [5 * 29 + 7]))[0].double())
    # bias gradient = sum over K of op(A), both storage forms
    assert torch.allclose(G.bias_grad(a.t().contiguous(), ta=True), a.sum(1)) and torch.allclose(G.bias_grad(a, ta=False), a.sum(1))
    # valid extents inside wider buffers: NaN behind them never reaches the reference
    ap = torch.full((40, 80), float("nan"), dtype=F64); ap[:37, :72] = a
    wp = torch.full((32, 80), float("nan"), dtype=F64); wp[:29, :72] = w
    Z2, _ = G.product(ap, wp, m_valid=37, n_valid=29, k_valid=72)
    assert torch.equal(Z2, Z)
    for ta, tb, A_, B_ in ((False, False, a, w.t().contiguous()), (True, False, a.t().contiguous(), w.t().contiguous())):
        assert torch.allclose(G.product(A_, B_, ta, tb)[0], Z, rtol=1e-13)


@pytest.mark.parametrize("act", ["gelu", "relu"])
def test_derivative_epilogue_is_autograd(act):
    """C = acc * act'(src) * dropout (+ addend) is what autograd sends back through act(src) * dropout for the upstream gradient acc."""
    acc, src = G.rnd((19, 24), 5).double(), G.rnd((19, 24), 6).double().requires_grad_(True)
    add = G.rnd((19, 24), 7).double()
    drop = (5, 3, 0.3)
    m = G.drop_mask(19, 24, drop)
    fn = torch.nn.functional.gelu if act == "gelu" else torch.relu
    (fn(src) * m).backward(acc)
    e = G.epilogue(acc, act=act, dact_src=src.detach(), drop=drop, addend=add)
    assert torch.allclose(e["out"], src.grad + add, rtol=1e-12, atol=1e-14)
    assert e["preact"] is acc


def _bounded(M, N, K, out_dtype, seed, **epi):
    a, w, b = _operands(M, N, K, seed, False)
    Mv, Nv = a.shape[0], w.shape[0]
    kw = {}
    if epi.get("bias"):
        kw["bias"] = b
    if epi.get("act"):
        kw["act"] = epi["act"]
    if epi.get("addend"):
        kw["addend"] = G.rnd((Mv, Nv), seed + 3, 1.0, out_dtype)
    if epi.get("dact"):
        kw["dact_src"] = G.rnd((Mv, Nv), seed + 4, 1.0, out_dtype)
    if epi.get("drop"):
        kw["drop"] = (11, 4, 0.3)
    Z, S = G.product(a, w)
    e = G.epilogue(Z, **kw)
    return a, w, kw, e, S


# every shape of the GPU file, clipped to its first 64 rows / columns (module docstring) and then taken once
SHAPES = sorted({(min(m, 64), min(n, 64), k) for m, n, k in G.gpu_file_shapes()})


def test_gpu_file_shape_list_is_complete():
    full = G.gpu_file_shapes()
    ks = {k for _, _, k in SHAPES}
    assert ks == {k for _, _, k in full}
    assert set(G.GENERAL_K) | set(G.SPLIT_K) | set(G.F32_K) | set(G.SKINNY_K) | set(G.PT_K) | set(G.GROUP_ROWS) <= ks
    assert len(full) > 300 and max(ks) == 8200


def test_correct_emulation_stays_inside_the_bounds_at_every_shape():
    worst = 0.0
    for i, (M, N, K) in enumerate(SHAPES):
        out_dtype = (BF, F32)[i % 2]
        a, w, kw, e, S = _bounded(M, N, K, out_dtype, 100 + i)
        got, _ = G.emulate(a, w, out_dtype=out_dtype, split=1 + i % 5, seed=i)
        bnd = G.bound(e["out"], S, K, out_dtype)
        excess = float(((got.double() - e["out"]).abs() - bnd).max())
        worst = max(worst, float(((got.double() - e["out"]).abs() / bnd).max()))
        assert excess <= 0.0, (M, N, K, out_dtype, excess)
        # integer operands: bit-exact in any split and order
        ai, wi, bi = _operands(M, N, K, 500 + i, True)
        goti, _ = G.emulate(ai, wi, bias=bi, out_dtype=out_dtype, split=1 + (i + 2) % 5, seed=i)
        Zi, _ = G.product(ai, wi)
        assert torch.equal(goti, (Zi + bi.double()).to(F32).to(out_dtype)), (M, N, K)
    print(f"[gemm] emulation: worst |delta| / bound over {len(SHAPES)} shapes = {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("out_dtype", [BF, F32])
@pytest.mark.parametrize("epi", [dict(bias=True), dict(bias=True, act="gelu"), dict(act="relu", addend=True), dict(bias=True, act="gelu", drop=True),
                                 dict(act="gelu", dact=True), dict(act="relu", dact=True, drop=True, addend=True)], ids=lambda e: "+".join(sorted(e)))
def test_correct_emulation_with_epilogues_stays_inside_the_bounds(out_dtype, epi):
    for i, (M, N, K) in enumerate([(65, 63, 8), (63, 65, 72), (33, 77, 203), (16, 72, 1000), (64, 64, 4096)]):
        a, w, kw, e, S = _bounded(M, N, K, out_dtype, 900 + i, **epi)
        got, pre = G.emulate(a, w, out_dtype=out_dtype, split=3, seed=i, **kw)
        G.check_elem(f"emulation {M}x{N}x{K}", got, e["out"], G.bound(e["out"], S, K, out_dtype, kw.get("bias"), kw.get("act"), e))
        G.check_elem(f"emulation {M}x{N}x{K} preact", pre, e["preact"], G.bound(e["preact"], S, K, out_dtype, kw.get("bias"), what="preact"))
        if epi.get("drop"):
            G.check_mask("emulation mask", got, e["out"])


CASES = [(65, 63, 8), (63, 65, 72), (130, 77, 203), (17, 72, 1000), (64, 64, 4096)]


@pytest.mark.parametrize("fault", G.FAULTS)
@pytest.mark.parametrize("out_dtype", [BF, F32], ids=["bf16", "fp32"])
def test_exact_check_rejects_every_seeded_fault(fault, out_dtype):
    """Integer operands: the exact check sees every fault, at every shape, in both output types (a truncated bf16 result only exists
    for bf16 output, and only where results need rounding, |Z| > 256: K >= 1000 here)."""
    for i, (M, N, K) in enumerate(CASES):
        if fault == "truncate_bf16" and (out_dtype != BF or K < 1000):
            continue
        if fault == "double_partial" and K <= 64:
            continue                                        # (a single K tile: the doubled partial is the whole product, seen below)
        a, w, b = G.ints((M, K), 40 + i, BF), G.ints((N, K), 50 + i, BF), G.ints((N,), 60 + i)
        Z, _ = G.product(a, w)
        ref = Z + b.double()
        good, _ = G.emulate(a, w, bias=b, out_dtype=out_dtype, split=3, seed=i)
        G.check_exact("correct", good, ref)
        bad, _ = G.emulate(a, w, bias=b, out_dtype=out_dtype, split=3, seed=i, fault=fault)
        if torch.equal(bad, good):
            # the seeded place happened to hold zeros (a zero operand, equal neighbours): move the seed, never skip the fault
            bad = next(x for x in (G.emulate(a, w, bias=b, out_dtype=out_dtype, split=3, seed=i + 100 * j, fault=fault)[0] for j in range(1, 20))
                       if not torch.equal(x, good))
        with pytest.raises(AssertionError):
            G.check_exact(f"{fault}", bad, ref)


@pytest.mark.parametrize("fault", [f for f in G.FAULTS if f != "truncate_bf16"])
def test_bound_check_rejects_the_seeded_faults_on_random_inputs(fault):
    """Random operands, fp32 output (2^-24 |ref| + the accumulation term): each fault moves at least one element past its bound.
    (bf16 output hides a single dropped K element inside its 2^-8 rounding allowance: that is what the exact-integer check is for.)"""
    hit = 0
    for i, (M, N, K) in enumerate(CASES):
        if fault == "double_partial" and K <= 64:
            continue
        a, w, kw, e, S = _bounded(M, N, K, F32, 700 + i, bias=True)
        bad, _ = G.emulate(a, w, out_dtype=F32, split=3, seed=i, fault=fault, **kw)
        with pytest.raises(AssertionError):
            G.check_elem(fault, bad, e["out"], G.bound(e["out"], S, K, F32, kw["bias"]))
        hit += 1
    assert hit >= 4


def test_truncation_is_rejected_by_the_bit_exact_check_only_where_rounding_happens():
    a, w = G.ints((64, 4096), 1, BF), G.ints((64, 4096), 2, BF)
    Z, _ = G.product(a, w)
    bad, _ = G.emulate(a, w, out_dtype=BF, fault="truncate_bf16")
    n = int((bad.double() != Z.to(F32).to(BF).double()).sum())
    # Z has a standard deviation of 4 sqrt(K) = 256: about a third of the results lie above 256, where bf16 keeps even integers only
    # (multiples of 4 above 512), and chopping differs from rounding for the ones whose dropped bits are above the half
    assert n > 100
    with pytest.raises(AssertionError):
        G.check_exact("truncate", bad, Z)


def test_mask_check_rejects_a_shifted_mask():
    a, w, kw, e, S = _bounded(33, 40, 72, BF, 800, bias=True, drop=True)
    good, _ = G.emulate(a, w, out_dtype=BF, **kw)
    G.check_mask("mask", good, e["out"])
    other = dict(kw, drop=(11, 4, 0.3))
    other["drop"] = (12, 4, 0.3)
    bad, _ = G.emulate(a, w, out_dtype=BF, **other)
    with pytest.raises(AssertionError):
        G.check_mask("mask", bad, e["out"])
    with pytest.raises(AssertionError):
        G.check_mask("mask", torch.roll(good, 1, dims=1), e["out"])
