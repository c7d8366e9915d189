"""Kernel-level tests (GPU) of the sample-stationary stack kernels -- vct_layer_ss_fwd, vct_layer_ss_bwd, vct_ss_pack -- through
ops.layer_ss_desc / layer_ss_fwd / layer_ss_bwd_desc / layer_ss_bwd / ss_pack, no model object, each saved tensor against the fp64
reference of the same operation (tests/layer_ss_ref.py, itself checked by tests/test_layer_ss_ref_cpu.py).

Harness.  Every output lives in an Arena pre-filled with NaN, 64 canary bytes on both sides of each tensor; everything a kernel must not
read holds NaN (rows of x / mem / feats past B * L, the x fields of later layers, embedding-table rows no id names, a chunk behind the
weight stream; key-id columns past L hold ids that would change the mask).  Every call runs twice on fresh arenas: the two arenas must
be byte-identical, every output finite, every canary intact.  Weights are random per layer (gamma != 1, beta != 0), inputs N(0, 1).

Bounds (none sized from the kernels under test):
  pure products (qkv, a, cq, ckv, ca, hpre, f; backward: d hpre) in STEP mode, per element:
        |got - ref| <= 2^-8 |ref| + (K + 1) 2^-24 (sum_k |a_k w_k| + |bias|)
      one bf16 rounding of the result + the worst-case fp32 accumulation error of K products and the bias in any order (d hpre: times
      |dropout * act'|, + 2^-20 |acc| for the fast GELU': Abramowitz-Stegun 7.1.26 <= 1.5e-7, v_exp / v_rcp at 1 ulp);
  o, co, h, n*.y, x (bf16 results that are no bare product), per ROW: TOL[bf16] = 1.5e-2 of tests/test_kernels_gpu.py
      (test_attention_fwd_bwd, test_gemm_epilogues, test_add_layernorm_fwd_bwd use it over the whole tensor);
  rstd, per element: TOL[fp32] = 2e-5 relative (fp32 arithmetic on the stored bf16 operands);
  mean, absolute per row: 2^-24 sum_c |s_c| (fp32 summation of 512 addends in any order, then the exact division by 512) + 2^-24 |mean|;
  chain mode (fp64 from the stack input), last layer's output and the final norm, per row: 2.5e-2 (test_fused_equals_unfused_schedule);
  backward tensors whose gradient stays in registers / LDS between stores (d f, d a, d qkv, d x, the partial rows), per row: 2.5e-2
      (test_fused_backward_equals_unfused_chain);
  dropout: the elements that are exactly zero in the kernel's tensor and not in the reference's, or the other way round, number 0."""
import math

import numpy as np
import pytest
import torch

import layer_ss_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
D, NH = 512, 8
BF, F32 = torch.bfloat16, torch.float32
NAN = float("nan")
CH = R.SS_CHUNK
TOL_BF16, TOL_F32, TOL_CHAIN, TOL_BWD = 1.5e-2, 2e-5, 2.5e-2, 2.5e-2
U24, U8 = 2.0 ** -24, 2.0 ** -8


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from vct_amd import ops as _ops
    return _ops


def rnd(*shape, seed, scale=1.0, dtype=F32):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(DEV)


def padded_rows(t, extra=4):
    """A copy of the rows of t with `extra` NaN rows behind them; returns the view of the real rows."""
    buf = torch.full((t.shape[0] + extra, t.shape[1]), NAN, dtype=t.dtype, device=DEV)
    buf[:t.shape[0]] = t
    return buf[:t.shape[0]]


class Arena:
    """Output memory of one launch: NaN everywhere (0xFF bytes), each tensor 16-byte aligned between two 64-byte canaries."""
    GUARD, CANARY = 64, 0xA5

    def __init__(self, nbytes=48 << 20):
        self.buf = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
        self.at, self.guards, self.outs = 0, [], {}

    def take(self, name, shape, dtype):
        n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
        t0 = self.at + self.GUARD
        end = t0 + n + self.GUARD
        assert end <= self.buf.numel(), "arena too small"
        self.buf[self.at:t0] = self.CANARY
        self.buf[t0 + n:end] = self.CANARY
        self.guards += [(self.at, t0), (t0 + n, end)]
        self.at = (end + 15) // 16 * 16
        t = self.buf[t0:t0 + n].view(dtype).view(*shape)
        self.outs[name] = t
        return t

    def check(self):
        for a, b in self.guards:
            assert bool((self.buf[a:b] == self.CANARY).all()), f"canary bytes {a}..{b} overwritten"
        for name, t in self.outs.items():
            bad = (~torch.isfinite(t.float())).nonzero()
            assert bad.numel() == 0, f"{name}: NaN / unwritten element at {bad[0].tolist()} ({bad.shape[0]} in all)"


# ---- comparisons: every element, every row ----------------------------------------------------------------------------------------------
def _cpu(t):
    return t.detach().to("cpu").to(torch.float64)


def check_elem(what, got, ref, S, K, extra=None):
    got, bound = _cpu(got), U8 * ref.abs() + (K + 1) * U24 * S + (0.0 if extra is None else extra)
    excess = (got - ref).abs() - bound
    worst = int(excess.argmax())
    r, c = divmod(worst, got.shape[1])
    print(f"[layer-ss] {what}: worst |delta| - bound = {float(excess.max()):.3e} at row {r} column {c}")
    assert float(excess.max()) <= 0.0, f"{what}: row {r} column {c}: got {float(got[r, c])!r}, reference {float(ref[r, c])!r}, bound {float(bound[r, c]):.3e}"


def check_rows(what, got, ref, tol):
    got = _cpu(got)
    if got.dim() == 1:
        got, ref = got[:, None], ref[:, None]
    num, den = (got - ref).norm(dim=1), ref.norm(dim=1)
    zero = den == 0                                       # a reference row that is exactly zero (fully masked): the kernel's must be too
    assert bool((num[zero] == 0).all()), f"{what}: row {int((zero & (num > 0)).nonzero()[0])} must be exactly zero"
    err = torch.where(zero, torch.zeros_like(num), num / torch.where(zero, torch.ones_like(den), den))
    r = int(err.argmax())
    print(f"[layer-ss] {what}: worst row {r}: {float(err[r]):.3e} (bound {tol:.1e})")
    assert float(err[r]) < tol, f"{what}: row {r}: relative error {float(err[r]):.3e} >= {tol:.1e}"


def check_mean(what, got, ref, sabs):
    excess = (_cpu(got) - ref).abs() - (U24 * sabs + U24 * ref.abs())
    r = int(excess.argmax())
    print(f"[layer-ss] {what}: worst |delta| - bound = {float(excess[r]):.3e} at row {r}")
    assert float(excess[r]) <= 0.0, f"{what}: row {r}: got {float(got[r])!r}, reference {float(ref[r])!r}"


def check_zeros(what, got, ref, tiny=None):
    """tiny: elements whose exact value is below the documented absolute error of the operation that produced them (see gelu_tiny):
    the kernel may hold 0 there; they are printed, and they stay in every value comparison."""
    a, b = _cpu(got) == 0, ref == 0
    bad = a != b
    if tiny is not None:
        print(f"[layer-ss] {what}: {int((tiny & ~b).sum())} non-zero reference elements below the activation's absolute error, {int((tiny & bad).sum())} of them 0 in the kernel")
        bad = bad & ~tiny
    n = int(bad.sum())
    print(f"[layer-ss] {what}: {int(b.sum())} zeros in the reference, {n} mismatches")
    assert n == 0, f"{what}: {n} elements zero in one and not in the other, first at (row, column) {bad.nonzero()[0].tolist()}"


def gelu_tiny(hpre):
    """The fast GELU (csrc/vct_common.h: erf by Abramowitz-Stegun 7.1.26, |error| <= 1.5e-7, evaluated in fp32 as 1 - poly * e, which is
    1 exactly once poly * e < 2^-25) has an absolute error of up to |x| (0.75e-7 + 2^-25) < 2^-22 |x|: below about x = -5 the exact
    value x Phi(x) is smaller than that and the kernel's result is -0.  Those elements (and only those) may be zero in the kernel."""
    hp = _cpu(hpre)
    return (R.act_fn("gelu", hp).abs() <= 2.0 ** -22 * hp.abs()) & (hp != 0)


# ---- weights, streams ---------------------------------------------------------------------------------------------------------------------
_W = {}


def make_layer(ff, cross, seed):
    key = (ff, cross, seed)
    if key not in _W:
        s, k = 1 / math.sqrt(D), seed * 100
        norm = lambda i: (1 + 0.2 * rnd(D, seed=k + i), 0.2 * rnd(D, seed=k + i + 1))
        w = dict(w_in=rnd(3 * D, D, seed=k + 1, scale=s, dtype=BF), b_in=rnd(3 * D, seed=k + 2, scale=0.2),
                 w_o=rnd(D, D, seed=k + 3, scale=s, dtype=BF), b_o=rnd(D, seed=k + 4, scale=0.2),
                 w1=rnd(ff, D, seed=k + 5, scale=s, dtype=BF), b1=rnd(ff, seed=k + 6, scale=0.2),
                 w2=rnd(D, ff, seed=k + 7, scale=1 / math.sqrt(ff), dtype=BF), b2=rnd(D, seed=k + 8, scale=0.2),
                 n1=norm(10), n3=norm(14))
        if cross:
            w.update(c_in=rnd(3 * D, D, seed=k + 20, scale=s, dtype=BF), cb_in=rnd(3 * D, seed=k + 21, scale=0.2),
                     c_o=rnd(D, D, seed=k + 22, scale=s, dtype=BF), cb_o=rnd(D, seed=k + 23, scale=0.2), n2=norm(12))
        _W[key] = w
    return _W[key]


def fwd_stream(ops, layers, ff, cross, lead=None):
    """The packed stream of the stack (+ one NaN chunk behind it) and every layer's first chunk, laid out by the reference's table."""
    per = ops.layer_ss_stream_chunks(ff, cross)
    assert per == 8 * (4 + (4 if cross else 0) + 2 * (ff // 512))
    at, blocks, firsts = 0, [], []
    if lead is not None:
        blocks.append((lead, 8, 0, False)); at = 8
    for w in layers:
        firsts.append(at)
        blocks += R.pack_blocks(R.fwd_stream_table(ff, cross, at), w)
        at += per
    dst = torch.full(((at + 1) * CH,), NAN, dtype=BF, device=DEV)
    ops.ss_pack(blocks, dst)
    return dst, firsts, per


def bwd_stream(ops, layers_top_first, ff):
    per = ops.layer_ss_bwd_stream_chunks(ff)
    assert per == 8 * (2 * (ff // 512) + 4)
    blocks = []
    for k, w in enumerate(layers_top_first):
        blocks += R.pack_blocks(R.bwd_stream_table(ff, k * per), w)
    dst = torch.full(((per * len(layers_top_first) + 1) * CH,), NAN, dtype=BF, device=DEV)
    ops.ss_pack(blocks, dst)
    return dst, per


def make_mask(kind, B, L):
    """(key_pad argument of the descriptors, causal, reference key mask [B, L] or None).  Sample 0 is never padded."""
    if kind == "none":
        return None, False, None
    if kind == "byte":            # [B, L] bytes, shift 0: sample 1 ragged, the LAST sample fully masked (the zero convention)
        m = torch.zeros(B, L, dtype=torch.uint8)
        if B > 1:
            m[1, L - (L // 3 + 1):] = 1
        m[B - 1] = 1
        m = m.to(DEV)
        return m, False, R.key_mask(B, L, key_pad=m)
    if kind == "raw":             # the raw frame mask [B, L - 1] with shift 1: sample 1 ragged, the last sample keeps only key 0
        m = torch.zeros(B, L - 1, dtype=torch.bool)
        if B > 1:
            m[1, (L - 1) // 2:] = True
        m[B - 1] = True
        m = m.to(DEV)
        return (m, 1), False, R.key_mask(B, L, key_pad=m, shift=1)
    assert kind == "ids"          # causal + token ids: sample 1 is padding after its first token, the last sample after half of them
    ids = torch.randint(2, 40, (B, L + 3), generator=torch.Generator().manual_seed(L))
    if B > 1:
        ids[1, 1:L] = 0
    ids[B - 1, (L + 1) // 2:L] = 0 if L > 1 else ids[B - 1, 0]
    ids[:, L:] = 5
    ids[0, L:] = 0                # columns past L: reading them would change a mask
    ids = ids.to(DEV)
    return ("ids", ids, 0), True, R.key_mask(B, L, key_ids=ids, pad_id=0)


SAVED = ["qkv", "o", "a", "n1.y", "n1.mean", "n1.rstd", "hpre", "h", "f", "n3.y", "n3.mean", "n3.rstd"]
SAVED_X = ["cq", "ckv", "co", "ca", "n2.y", "n2.mean", "n2.rstd"]


class Fwd:
    """One forward case: inputs built once, launched on a fresh arena per run()."""

    def __init__(self, ops, *, B=3, L, ff=1024, act="gelu", n_layers=1, last=True, Lm=0, mask="none", p=0.0, pro=0, feats_dtype=F32,
                 want_x_in=True, seed=11):
        self.ops, self.B, self.L, self.ff, self.act, self.nl, self.last, self.Lm, self.p, self.pro = ops, B, L, ff, act, n_layers, last, Lm, p, pro
        cross = self.cross = Lm > 0
        M = B * L
        self.layers = [make_layer(ff, cross, seed + l) for l in range(n_layers)]
        self.final = (1 + 0.2 * rnd(D, seed=seed + 90), 0.2 * rnd(D, seed=seed + 91)) if last else None
        self.key_pad, self.causal, kpm = make_mask(mask, B, L)
        self.seed_t = torch.tensor([seed * 7919 + 1], dtype=torch.int32, device=DEV) if p > 0 else None
        self.sites = [tuple(10 * l + i for i in range(1, 7)) for l in range(n_layers)]
        self.mem = padded_rows(rnd(B * Lm, D, seed=seed + 50, dtype=BF)) if cross else None
        self.cfg = R.Cfg(B, L, ff, act, Lm=Lm, mem=self.mem, causal=self.causal, kpm=kpm, seed=seed * 7919 + 1 if p > 0 else None, p=p)
        self.x_later = torch.full((M, D), NAN, dtype=BF, device=DEV)           # the x fields of layers after the first: never read
        lead = None
        if pro == 0:
            self.x = padded_rows(rnd(M, D, seed=seed + 51, dtype=BF))
        elif pro == 1:
            T = self.T = L - 1
            self.feats = padded_rows(rnd(B * T, D, seed=seed + 52, dtype=feats_dtype))
            self.want_x_in = want_x_in and feats_dtype == F32
            self.w_u, self.b_u = rnd(D, D, seed=seed + 53, scale=1 / math.sqrt(D), dtype=BF), rnd(D, seed=seed + 54, scale=0.2)
            self.pe = padded_rows(rnd(L, D, seed=seed + 55))
            lead = self.w_u
        else:
            V = 48
            g = torch.Generator().manual_seed(seed + 56)
            ids = torch.randint(2, 40, (B, L + 3), generator=g)
            if mask == "ids":
                ids = self.key_pad[1].cpu().clone()
            ids[:, L:] = 1                                                          # id 1 names a NaN row of the table: never read
            self.emb_ids = ids.to(DEV)
            table = rnd(V, D, seed=seed + 57)
            named = torch.zeros(V, dtype=torch.bool)
            named[ids[:, :L].reshape(-1)] = True
            table[~named.to(DEV)] = NAN
            self.table, self.pos, self.site_emb = table, padded_rows(rnd(L, D, seed=seed + 58)), 77
            if mask == "ids":
                self.key_pad = ("ids", self.emb_ids, 0)
        self.stream, self.firsts, self.per = fwd_stream(ops, self.layers, ff, cross, lead)

    def descs(self, ar):
        B, L, M, ff = self.B, self.L, self.B * self.L, self.ff
        out, x = [], (self.x if self.pro == 0 else ar.take("x", (M, D), BF))
        for l, w in enumerate(self.layers):
            t = lambda n, shape, dt=BF: ar.take(f"L{l}.{n}", shape, dt)
            norm = lambda tag, gb: (gb[0], gb[1], t(tag + ".y", (M, D)), t(tag + ".mean", (M,), F32), t(tag + ".rstd", (M,), F32))
            bias = dict(qkv=w["b_in"], o=w["b_o"], l1=w["b1"], l2=w["b2"])
            kw = {}
            sa = (t("qkv", (M, 3 * D)), t("o", (M, D)), t("a", (M, D)))
            n1 = norm("n1", w["n1"])
            if self.cross:
                bias.update(cq=w["cb_in"][:D], ckv=w["cb_in"][D:], co=w["cb_o"])
                kw = dict(cross=(t("cq", (M, D)), t("ckv", (B * self.Lm, 2 * D)), t("co", (M, D)), t("ca", (M, D))), n2=norm("n2", w["n2"]),
                          mem=self.mem, Lm=self.Lm)
            ffn = (t("hpre", (M, ff)), t("h", (M, ff)), t("f", (M, D)))
            n3 = norm("n3", w["n3"])
            nf = norm("nf", self.final) if (self.last and l == self.nl - 1) else None
            if l == 0 and self.pro == 1:
                x_in = ar.take("x_in", (B * self.T, D), BF) if self.want_x_in else None
                kw["frontend"] = (self.feats, x_in, self.b_u, self.pe)
            if l == 0 and self.pro == 2:
                kw["embed"] = (self.emb_ids, self.table, self.pos, self.site_emb)
            out.append(self.ops.layer_ss_desc(
                B=B, Lr=L, x=x if l == 0 else self.x_later, wpk=self.stream[(self.firsts[l] if l else 0) * CH:], nchunks=self.per, ff=ff,
                act=self.act, H=NH, bias=bias, sa=sa, n1=n1, ffn=ffn, n3=n3, nf=nf, causal=self.causal, key_pad=self.key_pad,
                seed=self.seed_t, p_drop=self.p, sites=self.sites[l], **kw))
        return out

    def run(self):
        """Two launches on fresh arenas -> the first arena's outputs, per layer, by the reference's names."""
        arenas = []
        for _ in range(2):
            ar = Arena()
            self.ops.layer_ss_fwd(self.descs(ar))
            torch.cuda.synchronize()
            ar.check()
            arenas.append(ar)
        assert torch.equal(arenas[0].buf, arenas[1].buf), "a second identical launch gave different bytes"
        o = arenas[0].outs
        names = SAVED + (SAVED_X if self.cross else [])
        got = [{n: o[f"L{l}.{n}"] for n in names} for l in range(self.nl)]
        if self.last:
            got[-1].update({n: o[f"L{self.nl - 1}.{n}"] for n in ("nf.y", "nf.mean", "nf.rstd")})
        return got, o

    def check(self):
        got, o = self.run()
        B, L, c = self.B, self.L, self.cfg
        # the stack input: given, or built by the prologue (checked here, then taken AS STORED by the step reference)
        if self.pro == 0:
            x_step = x_chain = self.x
        elif self.pro == 1:
            ref, x_in = R.frontend(self.feats, self.w_u, self.b_u, self.pe, B, self.T, round_u=True)
            check_rows("x (front end)", o["x"], ref, TOL_BF16)
            if self.want_x_in:
                assert torch.equal(_cpu(o["x_in"]), x_in), "x_in is not the bf16 rounding of the features"
            x_step, x_chain = o["x"], R.frontend(self.feats, self.w_u, self.b_u, self.pe, B, self.T)[0]
        else:
            ref = R.embed(self.emb_ids, self.table, self.pos, B, L, c.seed, self.site_emb, c.p)
            check_rows("x (embedding)", o["x"], ref, TOL_BF16)
            check_zeros("x (embedding)", o["x"], ref)
            x_step, x_chain = o["x"], ref
        step = R.stack_fwd(x_step, self.layers, c, self.sites, self.final, got=got)
        for l, (ref, S) in enumerate(step):
            g = got[l]
            for n in ["qkv", "a", "hpre", "f"] + (["cq", "ckv", "ca"] if self.cross else []):
                check_elem(f"layer {l} {n}", g[n], ref[n], S[n], self.ff if n == "f" else D)
            for n in ["o", "h"] + (["co"] if self.cross else []):
                check_rows(f"layer {l} {n}", g[n], ref[n], TOL_BF16)
            check_zeros(f"layer {l} h", g["h"], ref["h"], gelu_tiny(g["hpre"]) if self.act == "gelu" else None)
            for tag in ["n1", "n3"] + (["n2"] if self.cross else []) + (["nf"] if "nf.y" in g else []):
                check_rows(f"layer {l} {tag}.y", g[tag + ".y"], ref[tag + ".y"], TOL_BF16)
                check_mean(f"layer {l} {tag}.mean", g[tag + ".mean"], ref[tag + ".mean"], S[tag + ".mean"])
                check_rows(f"layer {l} {tag}.rstd", g[tag + ".rstd"], ref[tag + ".rstd"], TOL_F32)
        chain = R.stack_fwd(x_chain, self.layers, c, self.sites, self.final)[-1][0]
        check_rows("chain: last layer's output", got[-1]["n3.y"], chain["n3.y"], TOL_CHAIN)
        if self.last:
            check_rows("chain: final norm", got[-1]["nf.y"], chain["nf.y"], TOL_CHAIN)


# ---- forward ------------------------------------------------------------------------------------------------------------------------------
ENC_CASES = [
    dict(L=1, ff=512, mask="byte"),
    dict(L=2, ff=1024, mask="raw", act="relu"),
    dict(L=15, ff=1536, mask="raw", n_layers=2),
    dict(L=16, ff=2048, mask="byte", n_layers=3, last=False),
    dict(L=17, ff=512, mask="none", n_layers=4),
    dict(L=31, ff=1536, mask="byte", act="relu", n_layers=2, last=False),
    dict(L=32, ff=2048, mask="raw", n_layers=4),
    dict(L=17, ff=1024, mask="raw", n_layers=5),
    dict(L=16, ff=512, mask="none", n_layers=5, last=False),
    dict(L=32, ff=1024, mask="byte", n_layers=8),
    dict(L=17, ff=1024, mask="raw", B=1),
    dict(L=15, ff=1024, mask="raw", p=0.1, n_layers=2),
    dict(L=32, ff=1536, mask="byte", p=0.5, n_layers=2, act="relu"),
]


def _id(c):
    return "-".join(f"{k}{v}" for k, v in c.items())


@pytest.mark.parametrize("case", ENC_CASES, ids=_id)
def test_encoder_stack_forward(ops, case):
    Fwd(ops, **case).check()


DEC_CASES = [
    dict(L=1, Lm=1, ff=512),
    dict(L=16, Lm=2, ff=1024, act="relu", n_layers=2),
    dict(L=17, Lm=15, ff=1536, n_layers=2, last=False),
    dict(L=32, Lm=16, ff=2048, n_layers=4),
    dict(L=17, Lm=16, ff=1024, n_layers=5),
    dict(L=16, Lm=15, ff=512, n_layers=8, last=False),
    dict(L=32, Lm=2, ff=1024, B=1),
    dict(L=17, Lm=16, ff=1024, p=0.1, n_layers=2),
    dict(L=16, Lm=15, ff=1536, p=0.5),
]


@pytest.mark.parametrize("case", DEC_CASES, ids=_id)
def test_decoder_stack_forward(ops, case):
    """Causal self-attention with key padding from the token ids (sample 1 is padding after its first token), cross-attention over Lm rows."""
    Fwd(ops, mask="ids", **case).check()


PRO1_CASES = [dict(T=1, feats_dtype=F32), dict(T=15, feats_dtype=BF), dict(T=16, feats_dtype=F32, want_x_in=False),
              dict(T=31, feats_dtype=F32, n_layers=2), dict(T=16, feats_dtype=BF, n_layers=5, p=0.1)]


@pytest.mark.parametrize("case", PRO1_CASES, ids=_id)
def test_encoder_prologue(ops, case):
    """pro = 1: the unify Linear, the mean row and the PE' rows build x (the unify block leads the stream: every layer's chunks move by 8)."""
    case = dict(case)
    Fwd(ops, L=case.pop("T") + 1, ff=1024, mask="raw", pro=1, **case).check()


@pytest.mark.parametrize("case", [dict(L=1, p=0.0), dict(L=17, p=0.0, n_layers=2), dict(L=16, p=0.1), dict(L=32, p=0.5, n_layers=5)], ids=_id)
def test_decoder_prologue(ops, case):
    """pro = 2: ids with pads through the embedding table (rows no id names are NaN), positions, dropout with the embedding's own site."""
    Fwd(ops, Lm=15, ff=1024, mask="ids", pro=2, **case).check()


def test_more_samples_than_compute_units(ops):
    """B = 261 > 256 CUs: a compute unit takes a second workgroup."""
    Fwd(ops, B=261, L=5, ff=512, mask="raw").check()


# ---- backward -------------------------------------------------------------------------------------------------------------------------------
class Bwd:
    def __init__(self, ops, *, B=3, L, ff, n_layers=1, last=True, mask="none", p=0.0, act="gelu", seed=31):
        self.ops, self.B, self.L, self.ff, self.nl, self.last, self.p = ops, B, L, ff, n_layers, last, p
        M = B * L
        self.layers = [make_layer(ff, False, seed + l) for l in range(n_layers)]
        self.final = (1 + 0.2 * rnd(D, seed=seed + 90), 0.2 * rnd(D, seed=seed + 91)) if last else None
        self.key_pad, self.causal, kpm = make_mask(mask, B, L)
        sd = seed * 7919 + 3
        self.seed_t = torch.tensor([sd], dtype=torch.int32, device=DEV) if p > 0 else None
        self.cfg = c = R.Cfg(B, L, ff, act, causal=self.causal, kpm=kpm, seed=sd if p > 0 else None, p=p)
        self.act = act
        fs = [tuple(10 * l + i for i in range(1, 7)) for l in range(n_layers)]
        self.sites = [(s[0], s[1], s[4], s[5]) for s in fs]
        # the saved forward tensors: the fp64 reference (chain mode), rounded to bf16 -- NOT the fused forward's
        x = rnd(M, D, seed=seed + 51, dtype=BF)
        fwd = R.stack_fwd(x, self.layers, c, fs, self.final)
        dev = lambda t, dt=BF: padded_rows(t.to(dt).to(DEV)) if t.dim() == 2 else t.to(dt).to(DEV)
        self.saved, xin = [], x
        for out, _ in fwd:
            sv = dict(x=padded_rows(xin), qkv=dev(out["qkv"]), a=dev(out["a"]), x1=dev(out["n1.y"]), hpre=dev(out["hpre"]), f=dev(out["f"]))
            sv.update({k: dev(out[k], F32) for k in ("n1.mean", "n1.rstd", "n3.mean", "n3.rstd")})
            self.saved.append(sv)
            xin = out["n3.y"].to(BF).to(DEV)
        top = fwd[-1][0]
        self.y_last = dev(top["n3.y"])
        self.nf_stats = (dev(top["nf.mean"], F32), dev(top["nf.rstd"], F32)) if last else None
        self.dy = padded_rows(rnd(M, D, seed=seed + 60, dtype=BF))
        self.order = list(reversed(range(n_layers)))
        self.stream, self.per = bwd_stream(ops, [self.layers[l] for l in self.order], ff)

    def descs(self, ar):
        B, L, M = self.B, self.L, self.B * self.L
        out = []
        for k, l in enumerate(self.order):
            w, sv = self.layers[l], self.saved[l]
            t = lambda n, shape, dt=BF: ar.take(f"L{l}.{n}", shape, dt)
            outs = (t("df", (M, D)), t("dhpre", (M, self.ff)), t("da", (M, D)), t("dqkv", (M, 3 * D)))
            n3 = (w["n3"][0], sv["n3.mean"], sv["n3.rstd"], t("n3.ws", (B, 2, D), F32))
            n1 = (w["n1"][0], sv["n1.mean"], sv["n1.rstd"], t("n1.ws", (B, 2, D), F32))
            nf = (self.final[0], *self.nf_stats, ar.take("nf.ws", (B, 2, D), F32)) if (self.last and k == 0) else None
            out.append(self.ops.layer_ss_bwd_desc(
                B=B, Lr=L, wpk=self.stream[k * self.per * CH:], nchunks=self.per, ff=self.ff, act=self.act, H=NH, x=sv["x"], qkv=sv["qkv"],
                a=sv["a"], x1=sv["x1"], hpre=sv["hpre"], f=sv["f"], n1=n1, n3=n3, outs=outs, sites=self.sites[l], nf=nf,
                y_last=self.y_last if (self.last and k == 0) else None, dy=self.dy if k == 0 else None,
                dx=ar.take("dx", (M, D), BF) if k == self.nl - 1 else None, causal=self.causal, key_pad=self.key_pad, seed=self.seed_t,
                p_drop=self.p))
        return out

    def check(self):
        ops, B, c = self.ops, self.B, self.cfg
        arenas = []
        for _ in range(2):
            ar = Arena()
            ops.layer_ss_bwd(self.descs(ar))
            norms = [n for n in ar.outs if n.endswith(".ws")]          # the partial rows summed as the engine sums them
            table = torch.tensor([[ar.outs[n].data_ptr(), ar.take(n[:-2] + "dgamma", (D,), F32).data_ptr(),
                                   ar.take(n[:-2] + "dbeta", (D,), F32).data_ptr(), B] for n in norms], dtype=torch.int64, device=DEV)
            ops.ln_param_finalize_batched(table, len(norms), D)
            torch.cuda.synchronize()
            ar.check()
            arenas.append(ar)
        assert torch.equal(arenas[0].buf, arenas[1].buf), "a second identical launch gave different bytes"
        o = arenas[0].outs
        ref, nf_ws = R.stack_bwd(self.dy, self.saved, self.layers, c, self.sites, final=self.final[0] if self.last else None,
                                 y_last=self.y_last, nf_stats=self.nf_stats)

        def partial(what, got, want):
            check_rows(what + " partial rows (sample, dgamma | dbeta)", got.reshape(2 * B, D), want.reshape(2 * B, D), TOL_BWD)
            check_rows(what + " dgamma | dbeta", torch.stack([o[what + ".dgamma"], o[what + ".dbeta"]]), want.sum(0), TOL_BWD)
        if self.last:
            partial("nf", o["nf.ws"], nf_ws)
        for l in self.order:
            r, w, sv = ref[l], self.layers[l], self.saved[l]
            for n in ("df", "da", "dqkv"):
                check_rows(f"layer {l} {n}", o[f"L{l}.{n}"], r[n], TOL_BWD)
            val, S, acc = R.dhpre_step(o[f"L{l}.df"], sv["hpre"], w["w2"], c, self.sites[l][2])
            check_elem(f"layer {l} dhpre", o[f"L{l}.dhpre"], val, S, D, extra=2.0 ** -20 * acc)
            check_rows(f"layer {l} dhpre (chain)", o[f"L{l}.dhpre"], r["dhpre"], TOL_BWD)
            if self.p > 0 or self.act == "relu":
                check_zeros(f"layer {l} dhpre", o[f"L{l}.dhpre"], r["dhpre"])
            if self.p > 0:
                check_zeros(f"layer {l} df", o[f"L{l}.df"], r["df"])
                check_zeros(f"layer {l} da", o[f"L{l}.da"], r["da"])
            partial(f"L{l}.n3", o[f"L{l}.n3.ws"], r["n3.ws"])
            partial(f"L{l}.n1", o[f"L{l}.n1.ws"], r["n1.ws"])
        check_rows("dx", o["dx"], ref[0]["dx"], TOL_BWD)


BWD_CASES = [
    dict(L=1, ff=512, mask="none"),
    dict(L=15, ff=1536, mask="raw", n_layers=2),
    dict(L=16, ff=2048, mask="ids", n_layers=4, last=False),
    dict(L=17, ff=512, mask="raw", n_layers=2, p=0.3),
    dict(L=32, ff=1536, mask="ids", n_layers=4, p=0.3),
    dict(L=17, ff=2048, mask="byte", last=False, act="relu"),
    dict(L=32, ff=512, mask="none", n_layers=2, p=0.3, last=False, act="relu"),
]


@pytest.mark.parametrize("case", BWD_CASES, ids=_id)
def test_encoder_stack_backward(ops, case):
    Bwd(ops, **case).check()


# ---- vct_ss_pack ------------------------------------------------------------------------------------------------------------------------------
FILL = 0x7FC1          # a bf16 NaN pattern no weight holds: chunks no segment names must keep it


def _pack_and_compare(ops, host, blocks_spec, nchunks_dst):
    """blocks_spec: [(row0, col0, chunks, first chunk, transposed)] over the bf16 matrix `host` (any leading dimension)."""
    dst = torch.full((nchunks_dst * CH,), FILL, dtype=torch.int16, device=DEV).view(BF)
    ops.ss_pack([(host[r0:, c0:], nch, at, tr) for r0, c0, nch, at, tr in blocks_spec], dst)
    torch.cuda.synchronize()
    got = dst.view(torch.int16).cpu().numpy().reshape(nchunks_dst, 8, 4, 2, 64, 8)
    hb = host.view(torch.int16).cpu().numpy()
    named = np.zeros(nchunks_dst, bool)
    for r0, c0, nch, at, tr in blocks_spec:
        want = R.packed_block(hb[r0:, c0:], nch, tr)
        for c_ in range(nch):
            bad = np.argwhere(got[at + c_] != want[c_])
            assert bad.size == 0, f"block (rows {r0}.., columns {c0}.., transposed {tr}) chunk {c_}: first wrong (wave, tile, k-step, lane, j) = {bad[0].tolist()}"
        assert not named[at:at + nch].any()
        named[at:at + nch] = True
    assert bool((got[~named] == np.int16(FILL)).all()), "a chunk that no segment names was written"
    assert (~named).any()


def test_pack_transposed_and_strided(ops):
    big = rnd(1100, 1104 + 40, seed=5, dtype=BF)
    host = big[:, 16:16 + 1104]                                   # ldw 1144: not the row length
    _pack_and_compare(ops, host, [(104, 8, 3, 0, False), (64, 16, 4, 5, True), (0, 512, 8, 12, True), (512, 0, 2, 10, False)], 21)


def test_pack_fifty_segments_two_launches(ops):
    host = rnd(1024, 1024, seed=6, dtype=BF)
    order = np.random.default_rng(7).permutation(50)
    spec = [(64 * (i % 8), 64 * (i % 7), 1 + (i % 2), 3 * int(order[i]), bool(i % 3 == 0)) for i in range(50)]
    _pack_and_compare(ops, host, spec, 151)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------
def _refused(call, descs, arena, code):
    before = arena.buf.clone()
    with pytest.raises(ValueError, match=code):
        call(descs)
    torch.cuda.synchronize()
    assert torch.equal(before, arena.buf), "a refused call wrote to the arena"


def _all(field, value):
    def f(ds):
        for d in ds:
            setattr(d, field, value)
    return f


def _one(l, field, value):
    return lambda ds: setattr(ds[l], field, value)


def _bump(l, field, nbytes):
    return lambda ds: setattr(ds[l], field, getattr(ds[l], field) + nbytes)


FWD_REFUSALS = [
    ("enc", _all("ff", 256), "E_SHAPE"), ("enc", _all("ff", 2560), "E_SHAPE"), ("enc", _all("L", 33), "E_SHAPE"), ("dec", _all("Lm", 17), "E_SHAPE"),
    ("enc", _all("d", 256), "E_SHAPE"), ("enc", _all("H", 4), "E_SHAPE"), ("enc", _all("dtype", 0), "E_SHAPE"), ("dec", _all("Lm", 0), "E_SHAPE"),
    ("enc", _one(1, "L", 5), "E_ARG"), ("enc", _one(1, "causal", 1), "E_ARG"), ("enc", _one(1, "key_pad", 0), "E_ARG"),
    ("enc", _one(1, "seed", 0), "E_ARG"), ("enc", _one(1, "p_drop", 0.25), "E_ARG"), ("enc", _bump(1, "wpk", 65536), "E_ARG"),
    ("enc", _one(0, "last", 1), "E_ARG"), ("dec", _one(0, "pro", 1), "E_ARG"), ("enc", _one(0, "pro", 2), "E_ARG"),
    ("enc_pro", _one(1, "pro", 1), "E_ARG"), ("enc_pro", _all("L", 1), "E_ARG"), ("enc", _bump(0, "qkv", 2), "E_ALIGN"),
    ("dec", _bump(1, "ckv", 8), "E_ALIGN"), ("enc", _bump(0, "b1", 4), "E_ALIGN"),
]


@pytest.mark.parametrize("kind,mutate,code", FWD_REFUSALS, ids=[f"{i}-{k}-{c}" for i, (k, _, c) in enumerate(FWD_REFUSALS)])
def test_forward_refusals(ops, kind, mutate, code):
    """Valid two-layer descriptors (they are launched first: the unmutated call is accepted), one field changed -> the documented error,
    no byte of the arena touched."""
    case = dict(enc=dict(L=4, ff=512, mask="raw", p=0.1), dec=dict(L=4, Lm=3, ff=512, mask="ids"), enc_pro=dict(L=4, ff=512, mask="raw", pro=1))[kind]
    f = Fwd(ops, B=2, n_layers=2, **case)
    ar = Arena(8 << 20)
    descs = f.descs(ar)
    ops.layer_ss_fwd(descs)
    torch.cuda.synchronize()
    ar.check()
    mutate(descs)
    _refused(ops.layer_ss_fwd, descs, ar, code)


BWD_REFUSALS = [(4, _all("ff", 256), "E_SHAPE"), (4, _all("L", 33), "E_SHAPE"), (4, lambda ds: ds.append(ds[3]), "E_SHAPE"),
                (2, _one(0, "dy", 0), "E_ARG"), (2, _one(1, "dx", 0), "E_ARG"), (2, _one(1, "last", 1), "E_ARG"), (2, _one(1, "L", 5), "E_ARG"),
                (2, _bump(1, "wpk", 65536), "E_ARG"), (2, _bump(0, "df", 2), "E_ALIGN")]


@pytest.mark.parametrize("nl,mutate,code", BWD_REFUSALS, ids=[f"{i}-{c}" for i, (_, _, c) in enumerate(BWD_REFUSALS)])
def test_backward_refusals(ops, nl, mutate, code):
    b = Bwd(ops, B=2, L=4, ff=512, n_layers=nl, mask="raw", p=0.3)
    ar = Arena(8 << 20)
    descs = b.descs(ar)
    ops.layer_ss_bwd(descs)
    torch.cuda.synchronize()
    mutate(descs)
    _refused(ops.layer_ss_bwd, descs, ar, code)
