"""Unfused attention, CPU side: vct_attn_fwd / vct_attn_bwd validate their descriptor before any device use and answer with the codes
of include/vct_hip.h (one valid descriptor, one field changed per case; no case here reaches a launch), and the fp64 reference of the
GPU tests (tests/attn_ref.py) agrees with float64 autograd and with the H = 8 counter layout of layer_ss_ref.attn_drop."""
import ctypes
import math

import pytest
import torch

import attn_ref as A
import layer_ss_ref as R

E_ARG, E_SHAPE, E_ALIGN = -1, -2, -3


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from vct_amd import _lib
    return _lib.load()


_buf = (ctypes.c_float * 64)()
PTR = (ctypes.addressof(_buf) + 15) // 16 * 16          # dummy operand: non-null, 16-byte aligned, never dereferenced


def _desc(dtype, **changes):
    """A descriptor both entry points would accept (every operand of both directions set), then `changes`."""
    from vct_amd import _lib
    d = _lib.AttnDesc()
    d.dtype, d.B, d.H, d.Lq, d.Lk, d.hd = dtype, 2, 4, 6, 6, 16
    for f in ("q", "k", "v", "o", "d_o", "dq", "dk", "dv"):
        setattr(d, f, PTR)
    for f in ("ldq", "ldk", "ldv", "ldo", "ld_do", "ld_dq", "ld_dk", "ld_dv"):
        setattr(d, f, 64)
    for f, val in changes.items():
        setattr(d, f, val)
    return d


def _both(lib, d):
    return lib.vct_attn_fwd(d, None), lib.vct_attn_bwd(d, None)


@pytest.mark.parametrize("dtype", [0, 1], ids=["fp32", "bf16"])
def test_null_operands_and_bad_enums_are_arg_errors(lib, dtype):
    for f in ("q", "k", "v"):
        assert _both(lib, _desc(dtype, **{f: 0})) == (E_ARG, E_ARG), f
    for bad in (2, 7, -1):
        assert _both(lib, _desc(bad)) == (E_ARG, E_ARG), bad
    assert lib.vct_attn_fwd(_desc(dtype, o=0), None) == E_ARG
    for f in ("d_o", "dq", "dk", "dv"):
        assert lib.vct_attn_bwd(_desc(dtype, **{f: 0}), None) == E_ARG, f
    for f in ("q_bs", "k_bs", "v_bs", "o_bs"):               # strided batches: forward (decode) only
        assert lib.vct_attn_bwd(_desc(dtype, **{f: 6 * 64}), None) == E_ARG, f


@pytest.mark.parametrize("dtype", [0, 1], ids=["fp32", "bf16"])
def test_shapes_beyond_the_kernel_are_shape_errors(lib, dtype):
    for f in ("B", "H", "Lq", "Lk", "hd"):
        for val in (0, -1):
            assert _both(lib, _desc(dtype, **{f: val})) == (E_SHAPE, E_SHAPE), (f, val)
    for f, val in (("Lq", 65), ("Lk", 65), ("hd", 136)):
        assert _both(lib, _desc(dtype, **{f: val})) == (E_SHAPE, E_SHAPE), (f, val)
    assert _both(lib, _desc(dtype, key_pad_shift=-1)) == (E_SHAPE, E_SHAPE)
    assert _both(lib, _desc(dtype, key_pad=PTR, key_pad_shift=-1)) == (E_SHAPE, E_SHAPE)
    for shift in (6, 7):                                     # a mask row of width Lk - shift <= 0
        assert _both(lib, _desc(dtype, key_pad=PTR, key_pad_shift=shift)) == (E_SHAPE, E_SHAPE), shift


@pytest.mark.parametrize("dtype", [0, 1], ids=["fp32", "bf16"])
def test_misaligned_operands_are_align_errors(lib, dtype):
    vec = 8 if dtype == 1 else 4
    off = 64 - vec // 2                                      # a multiple of vec / 2 only: 60 (bf16), 62 (fp32)
    assert _both(lib, _desc(dtype, hd=16 - vec // 2)) == (E_ALIGN, E_ALIGN)
    for f in ("ldq", "ldk", "ldv"):
        assert _both(lib, _desc(dtype, **{f: off})) == (E_ALIGN, E_ALIGN), f
        assert _both(lib, _desc(dtype, **{f: 65})) == (E_ALIGN, E_ALIGN), f
    assert lib.vct_attn_bwd(_desc(dtype, ld_do=off), None) == E_ALIGN
    assert lib.vct_attn_fwd(_desc(dtype, ldo=62), None) == E_ALIGN     # outputs: four columns per store in either dtype
    for f in ("ld_dq", "ld_dk", "ld_dv"):
        assert lib.vct_attn_bwd(_desc(dtype, **{f: 62}), None) == E_ALIGN, f
    step = 4 if dtype == 1 else 8                            # bytes: half of the 8-byte (bf16) / 16-byte (fp32) output vector
    assert lib.vct_attn_fwd(_desc(dtype, o=PTR + step), None) == E_ALIGN
    for f in ("dq", "dk", "dv"):
        assert lib.vct_attn_bwd(_desc(dtype, **{f: PTR + step}), None) == E_ALIGN, f


# ---- the fp64 reference of tests/test_attention_kernels_gpu.py -----------------------------------------------------------------------
def _rand(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _heads(x, B, L, H):
    """A.heads without the detach: autograd follows it."""
    return x.reshape(B, L, H, x.shape[1] // H).transpose(1, 2)


@pytest.mark.parametrize("case", [(2, 3, 7, 5, 12, False, True), (2, 4, 19, 13, 64, False, False), (1, 2, 9, 9, 8, True, True),
                                  (2, 2, 6, 11, 16, True, False), (2, 2, 11, 6, 16, True, True)])
def test_explicit_backward_equals_float64_autograd(case):
    """No fully masked row, no dropout: torch.softmax and autograd are then the same function."""
    B, H, Lq, Lk, hd, causal, pad = case
    d = H * hd
    q, k, v, do = (_rand(B * L, d, seed=70 + i) for i, L in enumerate((Lq, Lk, Lk, Lq)))
    kpm = None
    if pad:
        kpm = torch.zeros(B, Lk, dtype=torch.bool)
        kpm[-1, Lk - 2:] = True
    qa, ka, va = (t.clone().requires_grad_(True) for t in (q, k, v))
    s = _heads(qa, B, Lq, H) @ _heads(ka, B, Lk, H).transpose(-1, -2) / math.sqrt(hd)
    s = s.masked_fill(A.masked(B, Lq, Lk, causal, kpm), float("-inf"))
    o = A.flat(torch.softmax(s, -1) @ _heads(va, B, Lk, H))
    o.backward(do)
    assert torch.allclose(A.forward(q, k, v, B, H, Lq, Lk, causal, kpm), o.detach(), rtol=1e-12, atol=1e-13)
    for name, got, want in zip(("dq", "dk", "dv"), A.backward(q, k, v, do, B, H, Lq, Lk, causal, kpm), (qa.grad, ka.grad, va.grad)):
        assert torch.allclose(got, want, rtol=1e-11, atol=1e-12), name


def test_backward_with_a_multiplier_equals_autograd_through_it():
    """The dropout multiplier is a constant factor of P: autograd through (softmax o M) V gives the same three gradients."""
    B, H, Lq, Lk, hd = 2, 3, 7, 5, 8
    q, k, v, do = (_rand(B * L, H * hd, seed=80 + i) for i, L in enumerate((Lq, Lk, Lk, Lq)))
    M = A.mult(5, 3, 0.5, B, H, Lq, Lk)
    assert 0.2 < float((M == 0).double().mean()) < 0.8 and float(M.max()) == 2.0
    qa, ka, va = (t.clone().requires_grad_(True) for t in (q, k, v))
    s = _heads(qa, B, Lq, H) @ _heads(ka, B, Lk, H).transpose(-1, -2) / math.sqrt(hd)
    o = A.flat((torch.softmax(s, -1) * M) @ _heads(va, B, Lk, H))
    o.backward(do)
    assert torch.allclose(A.forward(q, k, v, B, H, Lq, Lk, M=M), o.detach(), rtol=1e-12, atol=1e-13)
    for got, want in zip(A.backward(q, k, v, do, B, H, Lq, Lk, M=M), (qa.grad, ka.grad, va.grad)):
        assert torch.allclose(got, want, rtol=1e-11, atol=1e-12)


def test_fully_masked_rows_are_zero_and_contribute_nothing():
    B, H, L, hd = 2, 2, 5, 8
    q, k, v, do = (_rand(B * L, H * hd, seed=90 + i) for i in range(4))
    kpm = torch.zeros(B, L, dtype=torch.bool)
    kpm[1] = True
    p = A.probs(q, k, B, H, L, L, kpm=kpm)
    assert bool((p[1] == 0).all()) and torch.allclose(p[0].sum(-1), torch.ones(H, L, dtype=torch.float64))
    o = A.forward(q, k, v, B, H, L, L, kpm=kpm)
    dq, dk, dv = A.backward(q, k, v, do, B, H, L, L, kpm=kpm)
    for t in (o, dq, dk, dv):
        assert bool(torch.isfinite(t).all()) and bool((t[L:] == 0).all()) and bool((t[:L] != 0).any())


def test_probs_and_mult_equal_the_layer_reference_at_eight_heads():
    B, Lq, Lk = 2, 7, 5
    for seed, site, p in ((1234, 3, 0.1), (5, 0, 0.5), (77, 11, 0.3)):
        assert torch.equal(A.mult(seed, site, p, B, 8, Lq, Lk), R.attn_drop(seed, site, p, B, Lq, Lk).to(torch.float64))
    assert bool((A.mult(None, 3, 0.1, B, 8, Lq, Lk) == 1).all()) and bool((A.mult(5, 3, 0.0, B, 8, Lq, Lk) == 1).all())
    q, k = _rand(B * Lq, 512, seed=60), _rand(B * Lk, 512, seed=61)
    kpm = R.key_mask(B, Lk, key_pad=torch.tensor([[0, 0, 0, 0, 1], [0, 0, 0, 0, 0]], dtype=torch.uint8))
    assert torch.allclose(A.probs(q, k, B, 8, Lq, Lk, True, kpm), R.softmax_masked(q, k, B, Lq, Lk, True, kpm), rtol=0, atol=1e-14)


def test_mult_counter_runs_over_heads_then_queries_then_keys():
    """An odd row length: the pair that shares one hash straddles two rows, and element (b, h, q, k) is element
    ((b H + h) Lq + q) Lk + k of the flat stream, whatever H is."""
    B, H, Lq, Lk = 2, 3, 5, 7
    M = A.mult(9, 2, 0.5, B, H, Lq, Lk)
    flat = torch.from_numpy(R.drop_mult(9, 2, 0.5, torch.arange(B * H * Lq * Lk).numpy()))
    assert torch.equal(M.reshape(-1), flat.to(torch.float64))
    assert torch.equal(M[1, 2, 4, 6], flat[((1 * H + 2) * Lq + 4) * Lk + 6].to(torch.float64))
