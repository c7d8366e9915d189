"""Kernel-level tests (GPU) of the batch-1 decode block kernels (vct_decode_block: self-attention, cross-attention, feed-forward,
generator with the fused greedy selection), of vct_greedy_select and of vct_decode_gemv's attention prologues at the key-count
limits, each against the fp64 reference of the same operation (tests/decode_block_ref.py).

Bounds (all from the project, none from a kernel's output):
  2e-5   relative Frobenius, fp32 arithmetic on given inputs against fp64 (TOL[torch.float32] of test_kernels_gpu.py);
  1e-5   the published input vector x_out (test_decode_gemv_stages' bound for the same quantity);
  1 ulp  values rounded into the bf16 cache: |slot - ref| <= 2^-7 |ref| + 1e-6 per element; 6e-3 for the whole row;
  6e-3   where a bf16 rounding inside the kernel is NOT mirrored by the reference (cross-attention query, the chain).
The attention references take q and the fresh k | v from the kernel's own slot once the slot has passed its check, so the
scores and the partial out-projections are compared at fp32 tightness; the cross block keeps its query inside the kernel, so
its reference rounds the fp64 query to bf16 (tight bound) and is also evaluated unrounded (bf16 bound).

Every compute test calls the kernel twice (outputs and cache restored in between) and requires bit-identical outputs, intact
canaries around every output, and finite outputs although everything the kernel must not consume is NaN."""
import math

import numpy as np
import pytest
import torch

import decode_block_ref as R
from test_kernels_gpu import ref_attention

pytestmark = pytest.mark.gpu

DEV = "cuda"
D, H, HD, LMAX = 512, 8, 64, 64
CANARY = -777.25
NAN = float("nan")
BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from vct_amd import ops as _ops
    return _ops


def rnd(*shape, seed, scale=1.0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(DEV)


def rel(a, b):
    a = a.detach().double().cpu(); b = b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def check(what, err, bound):
    print(f"[decode-block] {what}: {err:.3e} (bound {bound:.0e})")
    assert err < bound, (what, err, bound)


def bits(t):
    return t.view(torch.int16) if t.dtype == BF16 else t


class Guard:
    """`n` rows of `cols` for a kernel to write, inside a canary-filled buffer (one row in front, two behind)."""

    def __init__(self, n, cols, dtype=torch.float32):
        self.n, self.buf = n, torch.empty(n + 3, cols, dtype=dtype, device=DEV)
        self.reset()

    def reset(self):
        self.buf.fill_(CANARY)

    @property
    def view(self):
        return self.buf[1:1 + self.n]

    def intact(self, valid_cols=None):
        ok = bool((self.buf[0] == CANARY).all()) and bool((self.buf[1 + self.n:] == CANARY).all())
        if valid_cols is not None:
            ok = ok and bool((self.view[:, valid_cols:] == CANARY).all())
        return ok


def run_twice(ops, kind, outs, guards, restore=None, **kw):
    """The launch, then the same launch again on re-canaried outputs (and a restored cache): bit-identical, finite outputs."""
    ops.decode_block(kind, D, **kw)
    first = [o.clone() for o in outs]
    for g in guards:
        g.reset()
    if restore is not None:
        restore()
    ops.decode_block(kind, D, **kw)
    torch.cuda.synchronize()
    for a, o in zip(first, outs):
        assert bool(torch.isfinite(o.float()).all()), "NaN / Inf reached an output"
        assert torch.equal(a, o), "a second identical call gave different bits"


@pytest.fixture(scope="module")
def wts():
    """One set of layer weights for every test: bf16 matrices in nn.Linear's [out, in] layout (+ the transposed copies the
    kernels read as w_b), fp32 biases and LayerNorm parameters."""
    ff = 2048
    w = dict(w_in=rnd(3 * D, D, seed=1, scale=1 / math.sqrt(D), dtype=BF16), b_in=rnd(3 * D, seed=2, scale=0.1),
             w_o=rnd(D, D, seed=3, scale=1 / math.sqrt(D), dtype=BF16),
             w1=rnd(ff, D, seed=4, scale=1 / math.sqrt(D), dtype=BF16), b1=rnd(ff, seed=5, scale=0.1),
             w2=rnd(D, ff, seed=6, scale=1 / math.sqrt(ff), dtype=BF16),
             ln1=(1 + 0.1 * rnd(D, seed=7), 0.1 * rnd(D, seed=8)), ln2=(1 + 0.1 * rnd(D, seed=9), 0.1 * rnd(D, seed=10)))
    w["w_o_t"] = w["w_o"].t().contiguous()
    w["w2_t"] = w["w2"].t().contiguous()
    return w


_GEN = {}


def gen_weights(V):
    """Generator weight / bias of a vocabulary size (cached: V = 30522 is 31 MB)."""
    if V not in _GEN:
        _GEN[V] = (rnd(V, D, seed=900 + V % 97, scale=1 / math.sqrt(D), dtype=BF16), rnd(V, seed=901 + V % 97, scale=0.1))
    return _GEN[V]


def make_source(kind, n_part=0, bias=False, seed=100):
    """Keyword arguments of the input vector (the same for ops.decode_block and the reference).  The buffer behind `part` holds
    NaN in its rows at or past n_part."""
    if kind == "embed":
        return dict(embed=(torch.tensor([37], dtype=torch.int64, device=DEV), rnd(50, D, seed=seed + 1), rnd(D, seed=seed + 2)))
    kw = dict(res=rnd(D, seed=seed + 3))
    if bias:
        kw["res_bias"] = rnd(D, seed=seed + 4, scale=0.1)
    if n_part:
        buf = torch.full((n_part + 4, D), NAN, device=DEV)
        buf[:n_part] = rnd(n_part, D, seed=seed + 5, scale=0.5)
        kw["part"] = buf[:n_part]
    return kw


# ---- input vector ------------------------------------------------------------------------------------------------------------------
SOURCES = [("embed", 0, False), ("res", 0, False), ("res", 0, True)] + [("res", n, b) for n in (1, 3, 8, 13, 32) for b in (False, True)]


@pytest.mark.parametrize("n_ln", [0, 1])
@pytest.mark.parametrize("src", SOURCES, ids=lambda s: f"{s[0]}-part{s[1]}-{'bias' if s[2] else 'nobias'}")
def test_input_vector_through_the_ffn_block(ops, wts, src, n_ln):
    """Embedded token or res (+ res_bias) (+ 1 .. 32 partial vectors, absent ones masked), no or one LayerNorm: the published
    x_out and the one partial row of an ff = 64 feed-forward block (one workgroup)."""
    kw = make_source(*src)
    if n_ln:
        kw["ln1"] = wts["ln1"]
    xo, po = Guard(1, D), Guard(1, D)
    w1, b1, w2, w2_t = wts["w1"][:64], wts["b1"][:64], wts["w2"][:, :64], wts["w2_t"][:64]
    run_twice(ops, "ffn", [xo.view, po.view], [xo, po], w_a=w1, b_a=b1, w_b=w2_t, ff=64, act="gelu", part_out=po.view,
              x_out=xo.view[0], **kw)
    x = R.input_vector(**kw)
    check("x_out", rel(xo.view[0], x), 1e-5)
    check("ffn partial", rel(po.view[0], R.ffn_block(x, w1, b1, w2, "gelu")[0]), 2e-5)
    assert xo.intact() and po.intact()


@pytest.mark.parametrize("src", [("embed", 0, False), ("res", 0, False), ("res", 13, True)], ids=lambda s: f"{s[0]}-part{s[1]}")
def test_input_vector_with_two_layernorms_through_the_generator(ops, wts, src):
    V, Vp = 127, 128
    kw = dict(make_source(*src), ln1=wts["ln1"], ln2=wts["ln2"])
    wg, bg = gen_weights(V)
    xo, lg = Guard(1, D), Guard(1, Vp)
    run_twice(ops, "gen", [xo.view, lg.view], [xo, lg], w_a=wg, b_a=bg, V=V, part_out=lg.view, x_out=xo.view[0], **kw)
    x = R.input_vector(**kw)
    check("x_out", rel(xo.view[0], x), 1e-5)
    check("logits", rel(lg.view[0, :V], R.gen_block(x, wg, bg)[0]), 2e-5)
    assert xo.intact() and lg.intact(V)


# ---- self-attention block ----------------------------------------------------------------------------------------------------------
def check_partials(what, got, want):
    for r in range(want.shape[0]):
        check(f"{what} partial row {r}", rel(got[r], want[r]), 2e-5)
    check(f"{what} sum of partials", rel(got.double().sum(0), want.sum(0)), 2e-5)


def check_slot(slot, want):
    """One bf16 ulp per element (a correct rounding is within half; one allows a rounding flipped by fp32 accumulation), then
    the project's bf16 bound on the row."""
    got = slot.double().cpu()
    excess = float(((got - want).abs() - (2.0 ** -7 * want.abs() + 1e-6)).max())
    print(f"[decode-block] slot: worst |delta| - (2^-7 |ref| + 1e-6) = {excess:.3e} (must be <= 0)")
    assert excess <= 0.0, excess
    check("slot row", rel(got, want), 6e-3)


@pytest.mark.parametrize("Lk", [1, 2, 9, 63, 64])
def test_self_attention_block(ops, wts, Lk):
    """Cache [64, 3d] with the slot in row Lk - 1 (as the engine's step passes it); rows at or past Lk - 1 are NaN before the call,
    the slot row included: the kernel overwrites it and never reads it."""
    kw = dict(make_source("res", 8, True, seed=200), ln1=wts["ln1"])
    cbuf = torch.full((LMAX + 2, 3 * D), NAN, dtype=BF16, device=DEV)
    cache = cbuf[1:1 + LMAX]
    cache[:Lk - 1] = rnd(Lk - 1, 3 * D, seed=210 + Lk, dtype=BF16)
    before = cbuf.clone()
    xo, po = Guard(1, D), Guard(H, D)
    run_twice(ops, "self", [xo.view, po.view, cache[Lk - 1]], [xo, po], restore=lambda: cbuf.copy_(before),
              w_a=wts["w_in"], b_a=wts["b_in"], slot=cache[Lk - 1], kc=cache[:, D:2 * D], vc=cache[:, 2 * D:], kv_ld=3 * D, Lk=Lk,
              w_b=wts["w_o_t"], part_out=po.view, x_out=xo.view[0], **kw)
    x = R.input_vector(**kw)
    check("x_out", rel(xo.view[0], x), 1e-5)
    slot = cache[Lk - 1].clone()
    proj, _ = R.self_block(x, wts["w_in"], wts["b_in"], cache[:Lk - 1, D:2 * D], cache[:Lk - 1, 2 * D:], wts["w_o"])
    check_slot(slot, proj)
    _, parts = R.self_block(x, wts["w_in"], wts["b_in"], cache[:Lk - 1, D:2 * D], cache[:Lk - 1, 2 * D:], wts["w_o"], qkv=slot)
    check_partials(f"self Lk={Lk}", po.view, parts)
    assert xo.intact() and po.intact()
    keep = torch.ones(LMAX + 2, dtype=torch.bool, device=DEV)
    keep[Lk] = False                                                            # (row Lk of the buffer = row Lk - 1 of the cache)
    assert torch.equal(bits(cbuf)[keep], bits(before)[keep]), "the cache changed outside the slot"


# ---- cross-attention block ---------------------------------------------------------------------------------------------------------
def bf16_boundary_distance(q):
    """The smallest distance of an element of q (fp64) to a value half-way between two neighbouring bf16 numbers.  The kernel's
    fp32 projection (512 products of magnitude ~0.03, eight in sequence and then a tree) is within about 2e-7 of the fp64 one;
    beyond ten times that, both round to the same bf16 value."""
    up = q.float().to(BF16).double()
    ulp = 2.0 ** (torch.floor(torch.log2(up.abs().clamp_min(1e-30))) - 7)
    return float((0.5 * ulp - (q - up).abs()).abs().min())


@pytest.mark.parametrize("Lk", [1, 13, 64])
def test_cross_attention_block(ops, wts, Lk):
    """w_a / b_a = the first d rows of a [3d, d] in-projection, memory K | V rows [*, 2d] with NaN at or past Lk, no slot."""
    kw = dict(make_source("res", 8, True, seed=325), ln1=wts["ln1"])
    kvbuf = torch.full((LMAX + 2, 2 * D), NAN, dtype=BF16, device=DEV)
    kvbuf[:Lk] = rnd(Lk, 2 * D, seed=310 + Lk, dtype=BF16)
    before = kvbuf.clone()
    w_q, b_q = wts["w_in"][:D], wts["b_in"][:D]
    xo, po = Guard(1, D), Guard(H, D)
    run_twice(ops, "cross", [xo.view, po.view], [xo, po], w_a=w_q, b_a=b_q, kc=kvbuf[:, :D], vc=kvbuf[:, D:], kv_ld=2 * D, Lk=Lk,
              w_b=wts["w_o_t"], part_out=po.view, x_out=xo.view[0], **kw)
    x = R.input_vector(**kw)
    check("x_out", rel(xo.view[0], x), 1e-5)
    # the query is rounded to bf16 inside the kernel and never stored: mirrored here for the fp32-tight comparison (the source's
    # seed keeps every element of the fp64 query away from a rounding boundary, so fp32 accumulation cannot flip one) ...
    assert bf16_boundary_distance(R.linear(x, w_q, b_q)) > 2e-6
    parts = R.cross_block(x, w_q, b_q, kvbuf[:Lk, :D], kvbuf[:Lk, D:], wts["w_o"], q_round=lambda q: q.float().to(BF16).double())
    check_partials(f"cross Lk={Lk}", po.view, parts)
    # ... and not mirrored under the project's bf16 bound
    plain = R.cross_block(x, w_q, b_q, kvbuf[:Lk, :D], kvbuf[:Lk, D:], wts["w_o"])
    for h in range(H):
        check(f"cross Lk={Lk} partial row {h} (unrounded query)", rel(po.view[h], plain[h]), 6e-3)
    assert xo.intact() and po.intact()
    assert torch.equal(bits(kvbuf), bits(before))


# ---- feed-forward block ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", ["gelu", "relu"])
@pytest.mark.parametrize("ff", [64, 192, 2048])
def test_feed_forward_block(ops, wts, ff, act):
    kw = dict(make_source("res", 8, True, seed=400), ln1=wts["ln1"])
    w1, b1, w2, w2_t = wts["w1"][:ff], wts["b1"][:ff], wts["w2"][:, :ff], wts["w2_t"][:ff]
    xo, po = Guard(1, D), Guard(ff // 64, D)
    run_twice(ops, "ffn", [xo.view, po.view], [xo, po], w_a=w1, b_a=b1, w_b=w2_t, ff=ff, act=act, part_out=po.view,
              x_out=xo.view[0], **kw)
    x = R.input_vector(**kw)
    check("x_out", rel(xo.view[0], x), 1e-5)
    check_partials(f"ffn ff={ff} {act}", po.view, R.ffn_block(x, w1, b1, w2, act))
    assert xo.intact() and po.intact()


# ---- generator and the fused selection ---------------------------------------------------------------------------------------------
class Sel:
    """Selection state of one caption with neighbours that must stay as they are: sel_ws (zeroed once) with a canary tail,
    tok_out / ended / ended_count / all_ended_at as the middle element of three."""

    def __init__(self, V, at=LMAX):
        self.nwg = (V + 127) // 128
        self.ws_buf = torch.full((2 * self.nwg + 1 + 8,), CANARY, device=DEV)
        self.ws = self.ws_buf[:2 * self.nwg + 1]
        self.ws.zero_()
        self.tok = torch.tensor([-7, -7, -7], dtype=torch.int64, device=DEV)
        self.ended = torch.tensor([9, 0, 9], dtype=torch.uint8, device=DEV)
        self.count = torch.tensor([9, 0, 9], dtype=torch.int32, device=DEV)
        self.at = torch.tensor([-9, at, -9], dtype=torch.int64, device=DEV)

    def args(self, end_id, t):
        return (self.ws, self.tok[1:2], end_id, self.ended[1:2], self.count[1:2], self.at[1:2], t)

    def state(self):
        """(token, ended, ended_count, all_ended_at) after checking the ticket and every neighbour."""
        torch.cuda.synchronize()
        assert int(self.ws[-1:].view(torch.int32)) == 0, "the ticket counter is not back at zero"
        assert bool((self.ws_buf[2 * self.nwg + 1:] == CANARY).all())
        assert self.tok.tolist()[::2] == [-7, -7] and self.ended.tolist()[::2] == [9, 9]
        assert self.count.tolist()[::2] == [9, 9] and self.at.tolist()[::2] == [-9, -9]
        return int(self.tok[1]), int(self.ended[1]), int(self.count[1]), int(self.at[1])


def first_argmax(row):
    return int(np.argmax(row.detach().float().cpu().numpy()))          # numpy: the first occurrence of the maximum


def gen_source(wts, seed=500):
    return dict(make_source("res", 13, True, seed=seed), ln1=wts["ln1"], ln2=wts["ln2"])


@pytest.mark.parametrize("select", [False, True], ids=["logits", "select"])
@pytest.mark.parametrize("V", [1, 127, 128, 129, 1000, 30522])
def test_generator_block(ops, wts, V, select):
    """Logits of a ragged last workgroup / fewer rows than one workgroup, columns [V, Vp) untouched; with the selection: the
    token is the first arg-max of the kernel's own logits and the fp64 reference's token (one bias entry is raised by 8, which
    puts the reference's top-2 margin far above 1e-3: nothing is skipped)."""
    Vp = (V + 31) // 32 * 32
    kw = gen_source(wts)
    wg, bg = gen_weights(V)
    bg = bg.clone()
    best = V - 1 if V % 128 == 1 else (5 * V) // 7
    bg[best] += 8.0
    lg = Guard(1, Vp)
    sel = Sel(V) if select else None
    run_twice(ops, "gen", [lg.view] + ([sel.tok] if select else []), [lg], w_a=wg, b_a=bg, V=V, part_out=lg.view,
              select=sel.args(-1, 3) if select else None, **kw)
    x = R.input_vector(**kw)
    want, tok, margin = R.gen_block(x, wg, bg)
    check(f"logits V={V}", rel(lg.view[0, :V], want), 2e-5)
    assert lg.intact(V)
    if select:
        assert margin >= 1e-3 and tok == best
        got = sel.state()
        assert got[0] == first_argmax(lg.view[0, :V]) == int(torch.max(lg.view[0, :V], 0)[1]) == tok
        assert got[1:] == (0, 0, LMAX)


@pytest.mark.parametrize("pair", [(130, 135), (130, 178), (5, 3 * 128 + 7), (0, 999)], ids=["lanes", "waves", "workgroups", "ends"])
def test_generator_selection_ties_give_the_first_index(ops, wts, pair):
    """Two rows with the same weights and bias (identical fp32 arithmetic -> identical logits) are the maxima: in two lanes of
    one wave, two waves of one workgroup, two workgroups, and rows 0 and V - 1."""
    V, Vp = 1000, 1024
    i, j = pair
    wg, bg = (a.clone() for a in gen_weights(V))
    wg[j] = wg[i]
    bg[i] += 8.0
    bg[j] = bg[i]
    lg, sel = Guard(1, Vp), Sel(V)
    run_twice(ops, "gen", [lg.view, sel.tok], [lg], w_a=wg, b_a=bg, V=V, part_out=lg.view, select=sel.args(-1, 3), **gen_source(wts))
    row = lg.view[0, :V]
    assert float(row[i]) == float(row[j]) == float(row.max()) and int((row == row.max()).sum()) == 2
    assert sel.state()[0] == i


def test_generator_selection_of_a_lone_last_row(ops, wts):
    """V % 128 == 1: the maximum is the only row of the last workgroup."""
    V, Vp = 257, 288
    wg, bg = gen_weights(V)
    bg = bg.clone()
    bg[V - 1] += 8.0
    lg, sel = Guard(1, Vp), Sel(V)
    run_twice(ops, "gen", [lg.view, sel.tok], [lg], w_a=wg, b_a=bg, V=V, part_out=lg.view, select=sel.args(-1, 3), **gen_source(wts))
    assert first_argmax(lg.view[0, :V]) == V - 1 and sel.state()[0] == V - 1 and lg.intact(V)


@pytest.mark.parametrize("previous", [LMAX, 2])
def test_generator_selection_bookkeeping(ops, wts, previous):
    V, Vp = 127, 128
    wg, bg = gen_weights(V)
    bg = bg.clone()
    bg[90] += 8.0
    lg, sel = Guard(1, Vp), Sel(V, at=previous)
    kw = dict(w_a=wg, b_a=bg, V=V, part_out=lg.view, **gen_source(wts))
    ops.decode_block("gen", D, select=sel.args(91, 3), **kw)                    # another token than end_id: nothing moves
    assert sel.state() == (90, 0, 0, previous)
    ops.decode_block("gen", D, select=sel.args(90, 5), **kw)                    # end_id: flag, count, all_ended_at = min(previous, t)
    assert sel.state() == (90, 1, 1, min(previous, 5))
    ops.decode_block("gen", D, select=sel.args(90, 1), **kw)                    # sticky: an ended caption changes nothing more
    assert sel.state() == (90, 1, 1, min(previous, 5))
    assert lg.intact(V)


def test_generator_selection_hand_off_over_32_launches(ops, wts):
    """32 launches in a row on ONE sel_ws with 32 different input vectors at V = 30522 (239 workgroups): every launch's token is
    the first arg-max of that launch's logits -- each launch must find the ticket at zero and read only pairs of its own
    workgroups.  One synchronisation, at the end."""
    V, Vp, n = 30522, 30528, 32
    wg, bg = gen_weights(V)
    res = rnd(n, D, seed=600)
    logits = torch.full((n, Vp), CANARY, device=DEV)
    toks = torch.full((n,), -7, dtype=torch.int64, device=DEV)
    sel = Sel(V)
    for i in range(n):
        ops.decode_block("gen", D, res=res[i], ln1=wts["ln1"], ln2=wts["ln2"], w_a=wg, b_a=bg, V=V, part_out=logits[i:i + 1],
                         select=(sel.ws, toks[i:i + 1], -1, sel.ended[1:2], sel.count[1:2], sel.at[1:2], i + 1))
    assert sel.state()[1:] == (0, 0, LMAX)
    want = np.argmax(logits[:, :V].cpu().numpy(), axis=1)
    assert toks.cpu().numpy().tolist() == want.tolist()
    assert len(set(want.tolist())) > 8                                          # (the inputs do tell the launches apart)
    assert bool((logits[:, V:] == CANARY).all())
    x = R.input_vector(res=res[n - 1], ln1=wts["ln1"], ln2=wts["ln2"])
    check("logits of the last launch", rel(logits[n - 1, :V], R.gen_block(x, wg, bg)[0]), 2e-5)


# ---- two layers + generator, wired as the engine's step ----------------------------------------------------------------------------
def test_chain_of_two_layers_and_the_generator(ops):
    """embed -> self -> cross -> ffn, the res / part / LayerNorm source into layer 2's self block, then the generator with two
    LayerNorms.  Reference: the fp64 composition of the pieces, nothing rounded; 6e-3 on the logits (the project's bf16 bound)
    because q | k | v pass through the bf16 cache in between."""
    ff, Lk, Te, V, Vp = 192, 9, 13, 1000, 1024
    s = iter(range(700, 800))

    def mat(o, i):
        return rnd(o, i, seed=next(s), scale=1 / math.sqrt(i), dtype=BF16)

    def vec(n):
        return rnd(n, seed=next(s), scale=0.1)

    def norm():
        return (1 + vec(D), vec(D))
    layers = []
    for _ in range(2):
        p = dict(sa_w=mat(3 * D, D), sa_b=vec(3 * D), sa_o=mat(D, D), sa_ob=vec(D), n1=norm(), ca_w=mat(3 * D, D), ca_b=vec(3 * D),
                 ca_o=mat(D, D), ca_ob=vec(D), n2=norm(), w1=mat(ff, D), b1=vec(ff), w2=mat(D, ff), b2=vec(D), n3=norm())
        p["cache"] = torch.full((LMAX, 3 * D), NAN, dtype=BF16, device=DEV)
        p["cache"][:Lk - 1] = rnd(Lk - 1, 3 * D, seed=next(s), dtype=BF16)
        p["kv"] = torch.full((Te + 3, 2 * D), NAN, dtype=BF16, device=DEV)
        p["kv"][:Te] = rnd(Te, 2 * D, seed=next(s), dtype=BF16)
        p["sa_o_t"], p["ca_o_t"], p["w2_t"] = (p[k].t().contiguous() for k in ("sa_o", "ca_o", "w2"))
        layers.append(p)
    nf, wg, bg = norm(), mat(V, D), vec(V)
    emb = (torch.tensor([11], dtype=torch.int64, device=DEV), rnd(50, D, seed=next(s)), rnd(D, seed=next(s)))
    caches = [p["cache"].clone() for p in layers]
    xa, x1, x2 = Guard(1, D), Guard(1, D), Guard(1, D)
    a_part, c_part, f_part, lg = Guard(H, D), Guard(H, D), Guard(ff // 64, D), Guard(1, Vp)
    guards = [xa, x1, x2, a_part, c_part, f_part, lg]

    def run():
        prev = None
        for p in layers:
            src = dict(embed=emb) if prev is None else dict(res=x2.view[0], res_bias=prev[0], part=f_part.view, ln1=prev[1])
            cache = p["cache"]
            ops.decode_block("self", D, w_a=p["sa_w"], b_a=p["sa_b"], slot=cache[Lk - 1], kc=cache[:, D:2 * D], vc=cache[:, 2 * D:],
                             kv_ld=3 * D, Lk=Lk, w_b=p["sa_o_t"], part_out=a_part.view, x_out=xa.view[0], **src)
            ops.decode_block("cross", D, res=xa.view[0], res_bias=p["sa_ob"], part=a_part.view, ln1=p["n1"], x_out=x1.view[0],
                             w_a=p["ca_w"][:D], b_a=p["ca_b"][:D], kc=p["kv"][:, :D], vc=p["kv"][:, D:], kv_ld=2 * D, Lk=Te,
                             w_b=p["ca_o_t"], part_out=c_part.view)
            ops.decode_block("ffn", D, res=x1.view[0], res_bias=p["ca_ob"], part=c_part.view, ln1=p["n2"], x_out=x2.view[0],
                             w_a=p["w1"], b_a=p["b1"], w_b=p["w2_t"], ff=ff, act="gelu", part_out=f_part.view)
            prev = (p["b2"], p["n3"])
        ops.decode_block("gen", D, res=x2.view[0], res_bias=prev[0], part=f_part.view, ln1=prev[1], ln2=nf, w_a=wg, b_a=bg, V=V,
                         part_out=lg.view)
        torch.cuda.synchronize()
        return lg.view[0, :V].clone()
    first = run()
    assert all(g.intact() for g in guards[:-1]) and lg.intact(V)
    for g in guards:
        g.reset()
    for p, c in zip(layers, caches):
        p["cache"].copy_(c)
    again = run()
    assert bool(torch.isfinite(first).all()) and torch.equal(first, again)
    # fp64 composition
    x, prev = R.input_vector(embed=emb), None
    for p, c in zip(layers, caches):
        if prev is not None:
            x = R.input_vector(res=x, res_bias=prev[0], part=prev[2], ln1=prev[1])
        _, a = R.self_block(x, p["sa_w"], p["sa_b"], c[:Lk - 1, D:2 * D], c[:Lk - 1, 2 * D:], p["sa_o"])
        y1 = R.input_vector(res=x, res_bias=p["sa_ob"], part=a, ln1=p["n1"])
        cc = R.cross_block(y1, p["ca_w"][:D], p["ca_b"][:D], p["kv"][:Te, :D], p["kv"][:Te, D:], p["ca_o"])
        x = R.input_vector(res=y1, res_bias=p["ca_ob"], part=cc, ln1=p["n2"])
        prev = (p["b2"], p["n3"], R.ffn_block(x, p["w1"], p["b1"], p["w2"], "gelu"))
    y = R.input_vector(res=x, res_bias=prev[0], part=prev[2], ln1=prev[1], ln2=nf)
    check("chain logits", rel(first, R.gen_block(y, wg, bg)[0]), 6e-3)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_unsupported_descriptors_are_refused(ops, wts):
    """Every one returns before any launch (the same codes at the C level: tests/test_abi_cpu.py)."""
    res = rnd(D, seed=800)
    big = torch.zeros(40, D, device=DEV)

    def ffn(ff, **kw):
        w = torch.zeros(ff, D, dtype=BF16, device=DEV)
        ops.decode_block("ffn", D, w_a=w, b_a=torch.zeros(ff, device=DEV), w_b=w, ff=ff, act="gelu", part_out=big, **kw)

    def attn(kind, Lk):
        cache = torch.zeros(LMAX + 2, 3 * D, dtype=BF16, device=DEV)
        ops.decode_block(kind, D, res=res, w_a=wts["w_in"][:3 * D if kind == "self" else D], b_a=wts["b_in"], w_b=wts["w_o_t"],
                         slot=cache[0] if kind == "self" else None, kc=cache[:, D:2 * D], vc=cache[:, 2 * D:], kv_ld=3 * D, Lk=Lk,
                         part_out=big)
    with pytest.raises(ValueError):
        ffn(64, res=res, part=torch.zeros(33, D, device=DEV))                   # more partial vectors than a prologue sums
    for ff in (2112, 96):
        with pytest.raises(ValueError):
            ffn(ff, res=res)
    for kind in ("self", "cross"):
        for Lk in (0, 65):
            with pytest.raises(ValueError):
                attn(kind, Lk)
    with pytest.raises(ValueError):                                             # d = 768
        w = torch.zeros(64, 768, dtype=BF16, device=DEV)
        ops.decode_block("ffn", 768, res=torch.zeros(768, device=DEV), w_a=w, b_a=torch.zeros(64, device=DEV), w_b=w, ff=64,
                         part_out=torch.zeros(4, 768, device=DEV))
    wg, bg = gen_weights(127)
    with pytest.raises(ValueError):
        ops.decode_block("gen", D, res=res, w_a=wg, b_a=bg, V=0, part_out=big)
    with pytest.raises(ValueError):                                             # g2 without g1
        ops.decode_block("gen", D, res=res, ln2=wts["ln2"], w_a=wg, b_a=bg, V=127, part_out=big)
    torch.cuda.synchronize()
    assert float(big.abs().sum()) == 0.0


# ---- vct_greedy_select -------------------------------------------------------------------------------------------------------------
def strided_logits(rows, cols, dtype, offset, seed, alternate=False):
    """x [rows, cols] as a view of rows `ldx` apart, ldx the first value above cols whose byte size is no multiple of 16 (so that
    not every row is 16-byte aligned: such a row takes the scalar scan; alternate: 8 modulo 16, i.e. even rows aligned and odd
    rows not), starting `offset` elements into the allocation.  The padding columns hold 1e30: scanning one would win."""
    es = 4 if dtype == torch.float32 else 2
    ldx = cols + 1
    while (ldx * es) % 16 == 0 or (alternate and (ldx * es) % 16 != 8):
        ldx += 1
    flat = torch.full((offset + rows * ldx,), 1e30, dtype=dtype, device=DEV)
    x = flat[offset:].view(rows, ldx)[:, :cols]
    x.copy_(rnd(rows, cols, seed=seed).to(dtype))
    return x


def select_state(rows, lmax=6):
    return (torch.full((rows, lmax), -1, dtype=torch.int64, device=DEV), torch.zeros(rows, dtype=torch.uint8, device=DEV),
            torch.zeros(1, dtype=torch.int32, device=DEV), torch.full((1,), lmax, dtype=torch.int64, device=DEV))


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("cols", [1, 7, 1000, 30522])
@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("dtype", [torch.float32, BF16])
def test_greedy_select_first_argmax(ops, dtype, rows, cols, offset):
    """Rows on the 16-byte vector scan and on the scalar scan in one call, `out` a column of the id matrix."""
    x = strided_logits(rows, cols, dtype, offset, seed=1000 + cols)
    aligned = [(x[r].data_ptr() % 16) == 0 for r in range(rows)]
    assert offset == 1 or aligned[0]
    assert rows == 1 or not all(aligned)
    ys, ended, count, at = select_state(rows)
    ops.greedy_select(x, ys[:, 2], -1, ended, count, at, 2, cols=cols)
    torch.cuda.synchronize()
    want = np.argmax(x.float().cpu().numpy(), axis=1)
    assert ys[:, 2].cpu().numpy().tolist() == want.tolist()
    assert bool((ys[:, :2] == -1).all()) and bool((ys[:, 3:] == -1).all())
    assert int(ended.sum()) == 0 and int(count) == 0 and int(at) == 6


@pytest.mark.parametrize("dtype", [torch.float32, BF16])
def test_greedy_select_ties_give_the_first_index(ops, dtype):
    cols = 30522
    vec = 4 if dtype == torch.float32 else 8
    tail = cols // vec * vec                                                    # the first column of an aligned row's scalar tail
    x = strided_logits(5, cols, dtype, 0, seed=1100, alternate=True)
    assert [x[r].data_ptr() % 16 == 0 for r in range(5)] == [True, False, True, False, True] and tail < cols
    ties = [(tail - 1, tail),                       # vector scan: its last element and the first one of the scalar tail
            (3, 1027),                              # scalar scan: two trips of one thread
            (100, cols - 1),                        # vector scan: one of its elements and the last one of the scalar tail
            (700, 1250),                            # scalar scan: the first index sits in a HIGHER wave (thread 700) than the second (226)
            (vec * 300, vec * 1250 + 1)]            # vector scan: the same (threads 300 and 226)
    for r, (i, j) in enumerate(ties):
        x[r, i] = x[r, j] = 99.0
    ys, ended, count, at = select_state(5)
    ops.greedy_select(x, ys[:, 1], -1, ended, count, at, 1, cols=cols)
    torch.cuda.synchronize()
    assert ys[:, 1].tolist() == [i for i, _ in ties]


@pytest.mark.parametrize("dtype", [torch.float32, BF16])
def test_greedy_select_end_of_sequence_bookkeeping(ops, dtype):
    """Three steps (and a later fourth) of MMT4Caption.greedy_decode's loop against a plain Python model of it: rows end at
    different steps, a row that emits end_id again is not counted twice, all_ended_at receives the step at which the last row
    ended and a later step does not raise it."""
    rows, cols, end_id, lmax = 5, 1000, 102, 6
    emits = {1: [0, 3], 2: [0, 1], 3: [2, 4], 4: [0, 1, 2, 3, 4]}               # rows whose arg-max is end_id at step t
    ys, ended, count, at = select_state(rows, lmax)
    end_flag, stop = [0] * rows, lmax                                           # the model: MMT4Caption.py's end_flag list and break
    for t in range(1, 5):
        x = strided_logits(rows, cols, dtype, 0, seed=1200 + t)
        x[:, end_id] = -50.0
        for r in emits[t]:
            x[r, end_id] = 50.0
        ops.greedy_select(x, ys[:, t], end_id, ended, count, at, t, cols=cols)
        torch.cuda.synchronize()
        next_word = np.argmax(x.float().cpu().numpy(), axis=1)
        for k, flag in enumerate((next_word == end_id).tolist()):
            if flag:
                end_flag[k] = 1
        if sum(end_flag) >= rows:
            stop = min(stop, t)
        assert ys[:, t].tolist() == next_word.tolist()
        assert ended.tolist() == end_flag and int(count) == sum(end_flag) and int(at) == stop, t
    assert stop == 3 and int(count) == rows


# ---- vct_decode_gemv: attention prologues at the key-count limits ------------------------------------------------------------------
@pytest.mark.parametrize("Lk", [1, 2, 63, 64])
@pytest.mark.parametrize("B", [1, 4])
@pytest.mark.parametrize("dtype", [torch.float32, BF16])
def test_decode_gemv_attention_prologues_at_the_key_count_limits(ops, dtype, B, Lk):
    """self_attn / cross_attn at 1, 2, 63 and 64 keys, cache rows at or past Lk NaN; bounds of test_decode_gemv_stages."""
    tol = 2e-5 if dtype == torch.float32 else 6e-3
    Wo = rnd(D, D, seed=1300, scale=1 / math.sqrt(D)).to(dtype)
    bo, res = rnd(D, seed=1301, scale=0.1), rnd(B, D, seed=1302)
    cache = rnd(B * LMAX, 3 * D, seed=1303 + Lk).to(dtype)
    c3 = cache.view(B, LMAX, 3 * D)
    c3[:, Lk:] = NAN
    slot = c3[:, Lk - 1]
    out = torch.full((B + 2, D), CANARY, device=DEV)
    ops.decode_gemv(Wo, out[1:1 + B], B, bias=bo, pro="self_attn",
                    attn=(slot[:, :D], cache[:, D:2 * D], cache[:, 2 * D:], 3 * D, LMAX * 3 * D, H, Lk), res=res)
    c64 = c3.double()
    att = ref_attention(c64[:, Lk - 1, :D].reshape(B, D), c64[:, :Lk, D:2 * D].reshape(B * Lk, D), c64[:, :Lk, 2 * D:].reshape(B * Lk, D),
                        B, H, 1, Lk, False, None)
    assert bool(torch.isfinite(out[1:1 + B]).all())
    check(f"gemv self_attn Lk={Lk}", rel(out[1:1 + B], att @ Wo.double().t() + bo.double() + res.double()), tol)
    kv = rnd(B * LMAX, 2 * D, seed=1310 + Lk).to(dtype)
    k3 = kv.view(B, LMAX, 2 * D)
    k3[:, Lk:] = NAN
    qc = rnd(B, D, seed=1320).to(dtype)
    out2 = torch.full((B + 2, D), CANARY, device=DEV)
    ops.decode_gemv(Wo, out2[1:1 + B], B, bias=bo, pro="cross_attn", attn=(qc, kv[:, :D], kv[:, D:], 2 * D, LMAX * 2 * D, H, Lk))
    k64 = k3.double()
    att = ref_attention(qc.double(), k64[:, :Lk, :D].reshape(B * Lk, D), k64[:, :Lk, D:].reshape(B * Lk, D), B, H, 1, Lk, False, None)
    assert bool(torch.isfinite(out2[1:1 + B]).all())
    check(f"gemv cross_attn Lk={Lk}", rel(out2[1:1 + B], att @ Wo.double().t() + bo.double()), tol)
    for o in (out, out2):
        assert bool((o[0] == CANARY).all()) and bool((o[1 + B:] == CANARY).all())
