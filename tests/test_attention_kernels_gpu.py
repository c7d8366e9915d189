"""Kernel-level tests (GPU) of the unfused attention -- vct_attn_fwd, vct_attn_bwd (csrc/vct_attn.hip, csrc/vct_attn_core.h) -- through
ops.attn_fwd / ops.attn_bwd, every output against the fp64 reference of the same operation (tests/attn_ref.py, itself checked by
tests/test_attention_refusals_cpu.py, which also holds the argument refusals).  THIS file owns the attention edges: the exact dropout
mask in both directions, the softmax range, head dimensions that need column padding, tile and wave edges, fully masked rows and the
KV-cache batch stride.  tests/test_kernels_gpu.py keeps the broad shapes (test_attention_fwd_bwd) and the three ways to state padding.

Harness.  Operands keep the real layout: q | k | v are column views of packed [rows, 3 d] buffers, dk | dv views of one buffer.  Every
column and row of those buffers that the launch must not read holds NaN (the k | v columns of the query buffer, the q columns of the
key buffer, rows behind the last one, cache rows at or beyond Lk); every output is a column view of a NaN buffer with guard columns
on both sides: the guards must still be NaN afterwards and every output element finite.

Bounds: the project's own (tests/test_kernels_gpu.py), relative Frobenius error against fp64 computed from the SAME rounded inputs:
fp32 2e-5 everywhere, bf16 1.5e-2 on the forward and 3e-2 on the gradients.  Each figure is printed before it is judged.
Dropout zero patterns: the elements that are zero in the kernel's tensor and not in the reference's, or the other way round, number 0.

Softmax range (group c): q, k on the grid of multiples of 1/8 in [-2, 2] (exact in bf16; every dot product, offset included, is exact
in fp32 accumulation), column 0 of k = 1 and of q = +-c, so every scaled score of a batch sits at or beyond +-100 while the
probabilities stay spread.  A plain float32 evaluation of the same formulas stays within 3.5e-6 of fp64 on o, dq, both parts of dk and
dv (checked on the CPU at head dimensions 24, 64, 96, 128): 2e-5 holds for a correct kernel.  Column 0 of each head of dk carries
c * scale * sum(dS) and is more than 100 times the norm of the other columns, so dk is judged twice: without those columns, and on
them alone."""
from types import SimpleNamespace

import pytest
import torch

import attn_ref as A

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF = torch.float32, torch.bfloat16
DTYPES = [F32, BF]
NAN = float("nan")
TOL_FWD = {F32: 2e-5, BF: 1.5e-2}
TOL_GRAD = {F32: 2e-5, BF: 3e-2}
OG, IG = 4, 8                    # guard columns of the output / dO buffers (pointers stay 16-byte (fp32) / 8-byte (bf16) aligned)


def _id(v):
    if isinstance(v, torch.dtype):
        return "fp32" if v == F32 else "bf16"
    if isinstance(v, tuple) and isinstance(v[0], tuple):       # (shape, causal)
        return _id(v[0]) + ("-causal" if v[1] else "")
    if isinstance(v, tuple):
        return "x".join(str(x) for x in v)
    return str(v)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from vct_amd import ops as _ops
    return _ops


def randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def grid8(*shape, seed):
    """Multiples of 1/8 in [-2, 2]."""
    return torch.randint(-16, 17, shape, generator=torch.Generator().manual_seed(seed)).float() / 8.0


def inputs(shape, seed=100):
    B, H, Lq, Lk, hd = shape
    d = H * hd
    return randn(B * Lq, d, seed=seed), randn(B * Lk, d, seed=seed + 1), randn(B * Lk, d, seed=seed + 2), randn(B * Lq, d, seed=seed + 3)


def seed_tensor(v):
    return torch.tensor([v], dtype=torch.int32, device=DEV)


def rel(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).norm() / ref.norm().clamp_min(1e-30))


def kpm_of(key_pad, B, Lk):
    if isinstance(key_pad, tuple) and key_pad[0] == "ids":
        return A.key_mask(B, Lk, key_ids=key_pad[1], pad_id=key_pad[2])
    return A.key_mask(B, Lk, key_pad=key_pad)


def pad_last(B, Lk, n=1):
    """uint8 [B, Lk]: the last n keys of the last batch are padded."""
    m = torch.zeros(B, Lk, dtype=torch.uint8, device=DEV)
    m[-1, Lk - n:] = 1
    return m


def _guarded(rows, cols, dtype, guard):
    buf = torch.full((rows, cols + 2 * guard), NAN, dtype=dtype, device=DEV)
    return buf, buf[:, guard:guard + cols]


def _check_guards(name, buf, cols, guard):
    assert bool(torch.isnan(buf[:, :guard]).all()) and bool(torch.isnan(buf[:, guard + cols:]).all()), f"{name}: a guard column was written"
    bad = (~torch.isfinite(buf[:, guard:guard + cols].float())).nonzero()
    assert bad.numel() == 0, f"{name}: NaN / unwritten element at {bad[0].tolist()} ({bad.shape[0]} in all)"


def run(ops, dtype, shape, q, k, v, do=None, causal=False, key_pad=None, dropout=None, cache=0):
    """One forward (and, with do, one backward) launch on the packed layout.  q, k, v, do: CPU fp32 values, rounded to dtype here.
    cache = Lmax: K | V live in a [B, Lmax, 3 d] cache whose rows at or beyond Lk hold NaN (forward only).  Returns the outputs
    (device) and the rounded operands (CPU fp64) the reference is computed from."""
    B, H, Lq, Lk, hd = shape
    d = H * hd
    bq = torch.full((B * Lq + 2, 3 * d), NAN, dtype=dtype, device=DEV)
    bq[:B * Lq, :d] = q.to(dtype)
    if cache:
        bk = torch.full((B * cache, 3 * d), NAN, dtype=dtype, device=DEV)
        kv3 = bk.view(B, cache, 3 * d)
        kv3[:, :Lk, d:2 * d] = k.to(dtype).view(B, Lk, d)
        kv3[:, :Lk, 2 * d:] = v.to(dtype).view(B, Lk, d)
        kv, stride = bk, cache * 3 * d
    else:
        bk = torch.full((B * Lk + 2, 3 * d), NAN, dtype=dtype, device=DEV)
        bk[:B * Lk, d:2 * d] = k.to(dtype)
        bk[:B * Lk, 2 * d:] = v.to(dtype)
        kv, stride = bk[:B * Lk], 0
    qv, kview, vview = bq[:B * Lq, :d], kv[:, d:2 * d], kv[:, 2 * d:]
    r = SimpleNamespace(q=q.to(dtype).double(), k=k.to(dtype).double(), v=v.to(dtype).double())
    bo, r.o = _guarded(B * Lq, d, dtype, OG)
    ops.attn_fwd(qv, kview, vview, r.o, B, H, Lq, Lk, causal=causal, key_pad=key_pad, dropout=dropout, kv_batch_stride=stride)
    torch.cuda.synchronize()
    _check_guards("o", bo, d, OG)
    if do is None:
        return r
    assert not cache
    bdo, dov = _guarded(B * Lq + 2, d, dtype, IG)
    dov[:B * Lq] = do.to(dtype)
    r.do = do.to(dtype).double()
    bdq, r.dq = _guarded(B * Lq, d, dtype, OG)
    bdkv, dkv = _guarded(B * Lk, 2 * d, dtype, OG)
    r.dk, r.dv = dkv[:, :d], dkv[:, d:]
    ops.attn_bwd(qv, kview, vview, dov[:B * Lq], r.dq, r.dk, r.dv, B, H, Lq, Lk, causal=causal, key_pad=key_pad, dropout=dropout)
    torch.cuda.synchronize()
    _check_guards("dq", bdq, d, OG)
    _check_guards("dk | dv", bdkv, 2 * d, OG)
    return r


def reference(r, shape, causal=False, key_pad=None, drop=None):
    """drop = (seed value, site, p).  Returns o, dq, dk, dv (fp64) and the probabilities P and multiplier M [B, H, Lq, Lk]."""
    B, H, Lq, Lk, hd = shape
    kpm = kpm_of(key_pad, B, Lk)
    M = A.mult(*drop, B, H, Lq, Lk) if drop is not None else None
    ref = SimpleNamespace(o=A.forward(r.q, r.k, r.v, B, H, Lq, Lk, causal, kpm, M), M=M, P=A.probs(r.q, r.k, B, H, Lq, Lk, causal, kpm),
                          masked=A.masked(B, Lq, Lk, causal, kpm).expand(B, H, Lq, Lk))
    if hasattr(r, "do"):
        ref.dq, ref.dk, ref.dv = A.backward(r.q, r.k, r.v, r.do, B, H, Lq, Lk, causal, kpm, M)
    return ref


def judge(tag, dtype, pairs):
    """pairs: (name, got, ref, bound).  Every figure is printed, then every one is asserted."""
    figs = [(name, rel(got, ref), bound) for name, got, ref, bound in pairs]
    for name, e, bound in figs:
        print(f"[attn] {tag} {_id(dtype)} {name}: {e:.3e} (bound {bound:.1e})")
    for name, e, bound in figs:
        assert e < bound, f"{tag} {name}: relative error {e:.3e} >= {bound:.1e}"


def judge_all(tag, dtype, r, ref):
    pairs = [("o", r.o, ref.o, TOL_FWD[dtype])]
    if hasattr(r, "dq"):
        pairs += [(n, getattr(r, n), getattr(ref, n), TOL_GRAD[dtype]) for n in ("dq", "dk", "dv")]
    judge(tag, dtype, pairs)


# ---- (a) dropout against the exact mask -----------------------------------------------------------------------------------------------
# one, two and three waves; odd Lk: one hash serves an element pair, and the pairs straddle the rows
DROP_CASES = [((2, 4, 19, 13, 64), False), ((1, 8, 30, 13, 96), False), ((2, 8, 39, 33, 128), False), ((2, 4, 17, 17, 32), True)]


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("case", DROP_CASES, ids=_id)
def test_dropout_against_the_exact_mask(ops, dtype, p, case):
    """o, dq, dk, dv against the reference built on the host replica of the counter hash: a wrong mask element in the forward, in
    backward phase A or in phase B, a missing 1 / (1 - p) on dP and a D built from the unmasked dP all show (fp32: one wrong element
    of the mask moves the error three orders of magnitude above the bound)."""
    shape, causal = case
    B, H, Lq, Lk, hd = shape
    key_pad = None
    if causal:                                                 # id padding at the tail: no row loses all of its keys
        ids = torch.randint(1, 90, (B, Lk + 1), generator=torch.Generator().manual_seed(7)).to(DEV)
        ids[0, 14:] = 0
        ids[1, 11:] = 0
        key_pad = ("ids", ids, 0)
    seed, site = 4321, 5
    q, k, v, do = inputs(shape)
    r = run(ops, dtype, shape, q, k, v, do, causal=causal, key_pad=key_pad, dropout=(seed_tensor(seed), site, p))
    ref = reference(r, shape, causal, key_pad, (seed, site, p))
    dropped = float((ref.M == 0).double().mean())
    assert abs(dropped - p) < 0.05, dropped
    judge_all(f"a/dropout p={p} {_id(shape)}", dtype, r, ref)


# ---- (b) mask read-out with an exact zero pattern ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("shape", [(2, 4, 19, 13, 64), (2, 8, 39, 33, 128)], ids=_id)
def test_dropout_mask_read_out(ops, dtype, shape):
    """V = [I | 0] per head makes o[:, :Lk] the forward's P o M itself, dO = [I | 0] makes dv[:, :Lq] the (P o M)^T that backward
    phase B regenerates: element by element the zeros must be the reference's zeros."""
    B, H, Lq, Lk, hd = shape
    d, p, seed, site = H * hd, 0.3, 99, 2
    assert Lk <= hd and Lq <= hd
    q, k, _, _ = inputs(shape, seed=200)
    v = torch.eye(Lk, hd).repeat(B, H)                         # row b * Lk + j, head h: unit vector j
    do = torch.eye(Lq, hd).repeat(B, H)
    key_pad = pad_last(B, Lk)
    r = run(ops, dtype, shape, q, k, v, do, key_pad=key_pad, dropout=(seed_tensor(seed), site, p))
    ref = reference(r, shape, False, key_pad, (seed, site, p))
    assert float(ref.P[~ref.masked].min()) > 1e-6              # no zero comes from underflow or rounding
    PM = ref.P * ref.M                                         # [B, H, Lq, Lk]
    assert 0.2 < float((PM[~ref.masked] == 0).double().mean()) < 0.4
    o4 = r.o.double().cpu().view(B, Lq, H, hd)
    dv4 = r.dv.double().cpu().view(B, Lk, H, hd)
    got_f, ref_f = o4[..., :Lk], PM.permute(0, 2, 1, 3)        # [B, Lq, H, Lk]
    got_b, ref_b = dv4[..., :Lq], PM.permute(0, 3, 1, 2)       # [B, Lk, H, Lq]
    wrong_f = int(((got_f == 0) != (ref_f == 0)).sum())
    wrong_b = int(((got_b == 0) != (ref_b == 0)).sum())
    print(f"[attn] b/read-out {_id(shape)} {_id(dtype)}: zero-pattern mismatches forward {wrong_f}, phase B {wrong_b}")
    assert wrong_f == 0 and wrong_b == 0
    assert bool((o4[..., Lk:] == 0).all()) and bool((dv4[..., Lq:] == 0).all())
    judge(f"b/read-out {_id(shape)}", dtype, [("P o M (forward)", got_f, ref_f, TOL_FWD[dtype]), ("P o M (phase B)", got_b, ref_b, TOL_GRAD[dtype]),
                                             ("dq", r.dq, ref.dq, TOL_GRAD[dtype]), ("dk", r.dk, ref.dk, TOL_GRAD[dtype])])


# ---- (c) softmax range --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("case", [((2, 4, 19, 13, 64), False), ((2, 8, 30, 33, 96), False), ((2, 4, 39, 39, 128), True)], ids=_id)
def test_softmax_range(ops, dtype, case):
    """Scores of batch 0 at or above +100, of batch 1 at or below -100: without the row maximum (or with a maximum that is not
    reduced over the four lane groups, or a phase B that rebuilds P from another maximum) exp overflows or every row underflows."""
    shape, causal = case
    B, H, Lq, Lk, hd = shape
    d = H * hd
    c = 1024.0 if hd <= 64 else 2048.0
    q, k = grid8(B * Lq, d, seed=300), grid8(B * Lk, d, seed=301)
    k.view(B * Lk, H, hd)[:, :, 0] = 1.0
    q.view(B, Lq, H, hd)[0, :, :, 0] = c
    q.view(B, Lq, H, hd)[1, :, :, 0] = -c
    v, do = randn(B * Lk, d, seed=302), randn(B * Lq, d, seed=303)
    r = run(ops, dtype, shape, q, k, v, do, causal=causal)
    assert torch.equal(r.q, q.double()) and torch.equal(r.k, k.double())      # the grid is exact in either dtype
    s = A.scores(r.q, r.k, B, H, Lq, Lk)
    assert float(s[0].min()) >= 100.0 and float(s[1].max()) <= -100.0
    ref = reference(r, shape, causal)
    dk3, rk3 = r.dk.double().cpu().view(B * Lk, H, hd), ref.dk.view(B * Lk, H, hd)
    assert float(rk3[..., 0].norm()) > 100.0 * float(rk3[..., 1:].norm())
    t = TOL_GRAD[dtype]
    judge(f"c/range {_id(shape)}", dtype, [("o", r.o, ref.o, TOL_FWD[dtype]), ("dq", r.dq, ref.dq, t), ("dk (columns 1..)", dk3[..., 1:], rk3[..., 1:], t),
                                          ("dk (column 0)", dk3[..., 0], rk3[..., 0], t), ("dv", r.dv, ref.dv, t)])


# ---- (d) head dimensions with column padding --------------------------------------------------------------------------------------------
HD_CASES = [(BF, hd) for hd in (8, 24, 40, 80, 120)] + [(F32, hd) for hd in (4, 12, 36, 68, 100, 124)]


@pytest.mark.parametrize("dtype,hd", HD_CASES, ids=[f"{_id(t)}-hd{hd}" for t, hd in HD_CASES])
@pytest.mark.parametrize("causal", [False, True], ids=["padded-19x13", "causal-33x33"])
def test_head_dimensions_with_column_padding(ops, dtype, hd, causal):
    """hd != 16 DT: the staging clamps the columns and zeroes them afterwards, the bf16 k-steps round up to 32 columns, the stores stop
    at hd.  The neighbours of a head's columns in the packed buffers are other heads or NaN."""
    shape = (1, 2, 33, 33, hd) if causal else (2, 3, 19, 13, hd)
    B, H, Lq, Lk, _ = shape
    key_pad = None
    if not causal:
        key_pad = pad_last(B, Lk, 2)
        key_pad[0, Lk - 1] = 1
    q, k, v, do = inputs(shape, seed=400)
    r = run(ops, dtype, shape, q, k, v, do, causal=causal, key_pad=key_pad)
    judge_all(f"d/head-dim {_id(shape)}", dtype, r, reference(r, shape, causal, key_pad))


# ---- (e) tile and wave edges -----------------------------------------------------------------------------------------------------------------
EDGE_CASES = [((2, 2, Lq, Lk, 32), False) for Lq, Lk in ((16, 16), (17, 16), (16, 17), (32, 33), (48, 49), (1, 50), (50, 1), (7, 64), (64, 7), (49, 5))]
EDGE_CASES += [((2, 2, 64, 64, 128), False), ((2, 2, 20, 33, 32), True), ((2, 2, 33, 20, 32), True)]


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("case", EDGE_CASES, ids=_id)
def test_tile_and_wave_edges(ops, dtype, case):
    """Sequence lengths at and next to the 16-row tile, one tile against four (the backward then runs four waves of which three skip a
    whole phase), the API maximum (its backward opts in to the large LDS), the causal mask (key > query) with Lq != Lk.  The last key of
    the last batch is padded (Lk = 1: that batch is then fully masked and all zero)."""
    shape, causal = case
    B, H, Lq, Lk, hd = shape
    key_pad = pad_last(B, Lk)
    q, k, v, do = inputs(shape, seed=500)
    r = run(ops, dtype, shape, q, k, v, do, causal=causal, key_pad=key_pad)
    judge_all(f"e/edges {_id(shape)}{' causal' if causal else ''}", dtype, r, reference(r, shape, causal, key_pad))


# ---- (f) fully masked rows --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("form", ["batch", "causal-ids"])
def test_fully_masked_rows_are_zero(ops, dtype, form):
    """m == -inf -> 0, inv = 0: the rows without a key are exactly zero in o and dq, every output is finite (run() checks it), and dk
    and dv are the reference's, to which those rows contribute nothing."""
    shape = B, H, Lq, Lk, hd = (2, 4, 19, 19, 64)
    if form == "batch":
        causal = False
        key_pad = torch.zeros(B, Lk, dtype=torch.uint8, device=DEV)
        key_pad[1] = 1
        rows = list(range(Lq, 2 * Lq))
    else:
        causal = True
        ids = torch.randint(1, 90, (B, Lk + 1), generator=torch.Generator().manual_seed(8)).to(DEV)
        ids[:, 0] = 0                                           # key 0 padded: query 0 sees nothing, every other query sees key 1..
        ids[1, 15:] = 0
        key_pad = ("ids", ids, 0)
        rows = [0, Lq]
    q, k, v, do = inputs(shape, seed=600)
    r = run(ops, dtype, shape, q, k, v, do, causal=causal, key_pad=key_pad)
    ref = reference(r, shape, causal, key_pad)
    dead = ref.masked.all(-1)                                  # [B, H, Lq], the same in every head
    assert [b * Lq + i for b, i in dead[:, 0].nonzero().tolist()] == rows and bool((dead == dead[:, :1]).all())
    assert bool((ref.o[rows] == 0).all()) and bool((ref.dq[rows] == 0).all())
    assert bool((r.o[rows] == 0).all()), "o of a fully masked row"
    assert bool((r.dq[rows] == 0).all()), "dq of a fully masked row"
    judge_all(f"f/masked-rows {form}", dtype, r, ref)


# ---- (g) KV cache stride (forward) --------------------------------------------------------------------------------------------------------------
LMAX = 56


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("LqLk", [(1, 1), (1, 16), (1, 17), (1, 50), (5, 20)], ids=_id)
def test_kv_cache_batch_stride(ops, dtype, LqLk):
    """K | V in a [B, Lmax, 3 d] cache, kv_batch_stride = Lmax * 3 d, the rows at or beyond Lk hold NaN: the decode step's layout.
    o is finite (run() checks it) and the reference's on the first Lk rows."""
    shape = (3, 4, *LqLk, 64)
    q, k, v, _ = inputs(shape, seed=700)
    r = run(ops, dtype, shape, q, k, v, cache=LMAX)
    judge_all(f"g/kv-cache {_id(shape)}", dtype, r, reference(r, shape))


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("Lk", [17, 50])
def test_kv_cache_dropout_counter_ignores_strides(ops, dtype, Lk):
    shape = (3, 4, 1, Lk, 64)
    seed, site, p = 31, 6, 0.1
    q, k, v, _ = inputs(shape, seed=700)
    strided = run(ops, dtype, shape, q, k, v, dropout=(seed_tensor(seed), site, p), cache=LMAX)
    packed = run(ops, dtype, shape, q, k, v, dropout=(seed_tensor(seed), site, p))
    assert torch.equal(strided.o, packed.o)
    ref = reference(strided, shape, drop=(seed, site, p))
    assert bool((ref.M == 0).any())
    judge_all(f"g/kv-cache dropout {_id(shape)}", dtype, strided, ref)
