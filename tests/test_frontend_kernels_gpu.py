"""Kernel-level tests (GPU) of the kernels between the data loader and the first encoder layer -- vct_enc_frontend_ex_fwd / _bwd,
vct_mm_frontend_fwd / _bwd, vct_enc_frontend_fwd / _bwd, vct_hmm_mix_fwd / _bwd, vct_gather_pad_rows, vct_cast and vct_transpose --
every element against the fp64 reference of the same operation and the derived per-element bounds of tests/frontend_ref.py (itself
checked by tests/test_frontend_ref_cpu.py, which also shows that each checker used here rejects the faults of frontend_ref.FAULTS).
Through vct_amd.ops wherever the wrapper takes the caller's output tensors; ops.gather_pad_rows allocates its own, so that entry point
is called through _lib.load() with the wrapper's argument order.

Harness.  Outputs live in an Arena (tests/gpu_arena.py) filled with 0xFF, 64 canary bytes on both sides of each.  NaN sits in everything
a kernel must not read: the rows of u behind B * T, the modal_w rows no label names, the emb_w rows no tidx names, temp / emb_w / modal_w
as a whole in the backward without the norm, beta in the backward, the store rows of clips that are not in idx and the rows behind the
store.  Every call runs twice on fresh arenas: the two must be byte-identical, every canary intact.  The dropout mask comes from
gemm_ref.drop_mask; none is read off a kernel.  The shapes are frontend_ref.SHAPES, which says beside each entry which loop trip it is
there for; the last test asserts that the cases that ran named every entry point in both types where it has two."""
import numpy as np
import pytest
import torch

import frontend_ref as F
from gpu_arena import Arena, up

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64, F32, BF, U8 = F.F64, F.F32, F.BF, torch.uint8
NAN = float("nan")
Z = F.SHAPES
TYPES = pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
RAN = set()                          # (entry point, dtype) of the calls whose judgement passed in this session
ENTRY_POINTS = {"vct_enc_frontend_ex_fwd": 2, "vct_enc_frontend_ex_bwd": 2, "vct_mm_frontend_fwd": 2, "vct_mm_frontend_bwd": 2,
                "vct_enc_frontend_fwd": 2, "vct_enc_frontend_bwd": 2, "vct_hmm_mix_fwd": 2, "vct_hmm_mix_bwd": 2,
                "vct_gather_pad_rows": 2, "vct_cast": 2, "vct_transpose": 1}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from vct_amd import ops as _ops
    return _ops


def guard(vals, extra=2):
    """vals [R, C] as the leading rows of a buffer with `extra` more rows of NaN behind it."""
    v = vals.to(DEV)
    buf = torch.full((v.shape[0] + extra, v.shape[1]), NAN, dtype=v.dtype, device=DEV)
    buf[:v.shape[0]] = v
    return buf[:v.shape[0]]


def nans(rows, cols, dtype=F32):
    return torch.full((rows, cols), NAN, dtype=dtype, device=DEV)


def dev(t):
    return None if t is None else t.to(DEV)


def mat(name, rows, cols, dtype, ld=None, skew=0):
    return (name, rows, cols, dtype, cols if ld is None else ld, skew)


def twice(build, nonfinite_ok=()):
    """build() -> arena: run on two fresh arenas; byte-identical, canaries intact, outputs finite.  Returns the first."""
    a1 = build()
    a2 = build()
    torch.cuda.synchronize()
    assert torch.equal(a1.buf, a2.buf), "two runs on fresh arenas differ"
    a1.check(nonfinite_ok)
    a2.check(nonfinite_ok)
    return a1


def report(capsys, what, worst):
    capsys.readouterr()
    with capsys.disabled():
        print(f"\n[front] {what}: kernels, worst |delta| / bound = {worst:.3f}")
    assert worst <= 1.0


class Dev:
    """The operands of a frontend_ref.Case on the device."""

    def __init__(self, c):
        self.us = [guard(u) for u in c.us]
        self.masks = None if c.masks is None else [dev(m) for m in c.masks]
        self.temp, self.emb_w, self.modal_w = dev(c.temp), dev(c.emb_w), dev(c.modal_w)
        self.tidx, self.labels = dev(c.tidx), dev(c.labels)
        self.gamma, self.beta, self.dx = dev(c.gamma), dev(c.beta), guard(c.dx)
        self.seed = torch.tensor([F.SEED], dtype=torch.int32, device=DEV)
        self.nan_temp, self.nan_emb = nans(c.S, c.d), nans(c.emb_rows, c.d)
        self.nan_modal = nans(c.n_labels, c.d) if c.n > 1 else None
        self.nan_beta = torch.full((c.d,), NAN, device=DEV)


# ---- vct_enc_frontend_ex ----------------------------------------------------------------------------------------------------------------------
def ex_fwd(ops, c, g, agg, learned, norm, p, key_pad=True):
    B, S, d, dt = c.B, c.S, c.d, c.dtype

    def build():
        specs = [mat("x0", B * S, d, dt)] + ([mat("key_pad", B, S, U8)] if key_pad else [])
        if norm:
            specs += [mat("mean", 1, B * S, F32), mat("rstd", 1, B * S, F32)]
        a = Arena(specs)
        kw = dict(agg=agg, modal_w=g.modal_w, labels=g.labels)
        kw.update(dict(tidx=g.tidx, emb_w=g.emb_w) if learned else dict(temp=g.temp))
        if norm:
            kw["norm"] = dict(gamma=g.gamma, beta=g.beta, mean=a["mean"], rstd=a["rstd"], dropout=None if p is None else (g.seed, F.SITE, p))
        ops.enc_frontend_ex_fwd(g.us, g.masks, a["x0"], a["key_pad"] if key_pad else None, B, c.Ts, **kw)
        return a
    a = twice(build)
    got = dict(x0=a["x0"], key_pad=a["key_pad"] if key_pad else None)
    if norm:
        got.update(mean=a["mean"], rstd=a["rstd"])
    return got, a


def ex_bwd(ops, c, g, ref, agg, learned, norm, p):
    """The backward on the reference's statistics rounded to fp32; what it need not read is NaN."""
    B, S, d, dt, n = c.B, c.S, c.d, c.dtype, c.n
    mean = rstd = None
    if norm:
        mean, rstd = dev(ref["mean32"]), dev(ref["rstd32"])

    def build():
        specs = [mat(f"du{i}", B * t, d, dt) for i, t in enumerate(c.Ts)]
        if n > 1:
            specs.append(mat("d_modal", c.n_labels, d, F32))
        if learned:
            specs.append(mat("d_emb", c.emb_rows, d, F32))
        if norm:
            specs += [mat("dpre", B * S, d, F32), mat("ws", B * n * 2, d, F32)]
        a = Arena(specs)
        kw = dict(agg=agg, labels=g.labels, modal_w=g.modal_w if norm else g.nan_modal)
        if learned:
            kw.update(tidx=g.tidx, emb_w=g.emb_w if norm else g.nan_emb, d_emb=a["d_emb"])
        else:
            kw.update(temp=g.temp if norm else g.nan_temp)
        if n > 1:
            kw["d_modal"] = a["d_modal"]
        if norm:
            kw.update(norm=dict(gamma=g.gamma, beta=g.nan_beta, mean=mean, rstd=rstd, dropout=None if p is None else (g.seed, F.SITE, p)),
                      dpre=a["dpre"], param_ws=a["ws"])
        ops.enc_frontend_ex_bwd(g.dx, [a[f"du{i}"] for i in range(n)], B, c.Ts, us=g.us if (norm or agg == "max") else None, **kw)
        return a
    a = twice(build)
    got = dict(du=[a[f"du{i}"] for i in range(n)])
    for k in ("d_modal", "d_emb", "dpre", "ws"):
        if k in a.outs:
            got[k] = a[k]
    return got, a


def run_ex(ops, dtype, only, capsys):
    worst, count = 0.0, 0
    for tag, c, combos, p, exact in F.ex_cases(dtype, only):
        g = Dev(c)
        for agg, learned, norm in combos:
            what = f"ex {tag} {agg} {'learned' if learned else 'fixed'} {'norm' if norm else 'plain'}"
            ref = F.reference(c, agg, learned, norm, F.drop_of(p))
            got, _ = ex_fwd(ops, c, g, agg, learned, norm, p)
            worst = max(worst, F.judge(what + " fwd", got, ref, c, agg, norm))
            got, _ = ex_bwd(ops, c, g, ref, agg, learned, norm, p)
            worst = max(worst, F.judge(what + " bwd", got, ref, c, agg, norm, exact))
            count += 1
    assert count > 0
    RAN.update({("vct_enc_frontend_ex_fwd", dtype), ("vct_enc_frontend_ex_bwd", dtype)})
    report(capsys, f"enc_frontend_ex {only} ({count} option combinations)", worst)


EX_GROUPS = ["regs", "no masks", "lane wrap", "zero slices", "S=1024", "first-reader scan", "out of range", "dropout", "mean 1000", "ties"]


@TYPES
@pytest.mark.parametrize("only", EX_GROUPS)
def test_enc_frontend_ex(ops, dtype, only, capsys):
    run_ex(ops, dtype, only, capsys)


@TYPES
def test_enc_frontend_ex_without_key_pad_and_with_p_zero(ops, dtype):
    """key_pad = None writes nothing else; p = 0 with a seed is bit-identical to no dropout (forward and backward)."""
    import ctypes
    from vct_amd import _lib as L
    from vct_amd.ops import frontend as FE
    r = Z["ex_regs"]
    c = F.Case(dtype, r["Ts"], r["B"], 72, seed=90)
    g = Dev(c)
    B, S, d, n = c.B, c.S, c.d, c.n
    ref = F.reference(c, "max", True, True)
    got, a = ex_fwd(ops, c, g, "max", True, True, None)
    got2, a2 = ex_fwd(ops, c, g, "max", True, True, None, key_pad=False)
    assert torch.equal(got["x0"], got2["x0"]) and torch.equal(got["mean"], got2["mean"]) and torch.equal(got["rstd"], got2["rstd"])
    F.judge("ex no key_pad", got2, ref, c, "max", True)
    b, _ = ex_bwd(ops, c, g, ref, "max", True, True, None)
    mean, rstd = dev(ref["mean32"]), dev(ref["rstd32"])

    def build():
        ar = Arena([mat("x0", B * S, d, dtype), mat("key_pad", B, S, U8), mat("mean", 1, B * S, F32), mat("rstd", 1, B * S, F32)]
                   + [mat(f"du{i}", B * t, d, dtype) for i, t in enumerate(c.Ts)]
                   + [mat("d_modal", c.n_labels, d, F32), mat("d_emb", c.emb_rows, d, F32), mat("dpre", B * S, d, F32), mat("ws", B * n * 2, d, F32)])
        norm = dict(gamma=g.gamma, beta=g.beta, mean=ar["mean"], rstd=ar["rstd"], dropout=None)
        desc = FE._fx_desc(dtype, B, d, c.Ts, "max", None, g.emb_w, g.tidx, g.modal_w, g.labels, norm)
        desc.seed, desc.site, desc.p_drop = g.seed.data_ptr(), F.SITE, 0.0
        for i, u in enumerate(g.us):
            desc.u[i] = u.data_ptr()
            desc.mask[i] = g.masks[i].data_ptr()
            desc.du[i] = ar[f"du{i}"].data_ptr()
        desc.x0, desc.key_pad = ar["x0"].data_ptr(), ar["key_pad"].data_ptr()
        L.check(L.load().vct_enc_frontend_ex_fwd(ctypes.byref(desc), L.stream_ptr()), "fwd")
        desc.mean, desc.rstd = mean.data_ptr(), rstd.data_ptr()
        desc.dx, desc.d_modal, desc.d_emb = g.dx.data_ptr(), ar["d_modal"].data_ptr(), ar["d_emb"].data_ptr()
        desc.dpre, desc.param_ws = ar["dpre"].data_ptr(), ar["ws"].data_ptr()
        L.check(L.load().vct_enc_frontend_ex_bwd(ctypes.byref(desc), L.stream_ptr()), "bwd")
        return ar
    ar = twice(build)
    for k in ("x0", "key_pad"):
        assert torch.equal(ar[k], got[k]), k
    for k in ("d_modal", "d_emb", "dpre", "ws"):
        assert torch.equal(ar[k], b[k]), k
    for i in range(n):
        assert torch.equal(ar[f"du{i}"], b["du"][i])


# ---- vct_mm_frontend ----------------------------------------------------------------------------------------------------------------------------
@TYPES
def test_mm_frontend(ops, dtype, capsys):
    worst = 0.0
    for tag, c, exact, both in F.mm_cases(dtype):
        g = Dev(c)
        B, S, d, n = c.B, c.S, c.d, c.n
        ref = F.reference(c, "avg", False, False)
        for key_pad in ((True, False) if tag == "no masks" else (True,)):
            def fwd():
                a = Arena([mat("x0", B * S, d, dtype)] + ([mat("key_pad", B, S, U8)] if key_pad else []))
                ops.mm_frontend_fwd(g.us, g.masks, g.temp, g.modal_w, g.labels, a["x0"], a["key_pad"] if key_pad else None, B, c.Ts)
                return a
            a = twice(fwd)
            worst = max(worst, F.judge(f"mm {tag} fwd", dict(x0=a["x0"], key_pad=a["key_pad"] if key_pad else None), ref, c, "avg", False))

        def bwd():
            ar = Arena([mat(f"du{i}", B * t, d, dtype) for i, t in enumerate(c.Ts)] + [mat("d_modal", c.n_labels, d, F32)])
            ops.mm_frontend_bwd(g.dx, [ar[f"du{i}"] for i in range(n)], ar["d_modal"], g.labels, B, c.Ts)
            return ar
        ab = twice(bwd)
        worst = max(worst, F.judge(f"mm {tag} bwd", dict(du=[ab[f"du{i}"] for i in range(n)], d_modal=ab["d_modal"]), ref, c, "avg", False, exact))
        if both:            # the shipped combination of enc_frontend_ex: the same bits
            e, _ = ex_fwd(ops, c, g, "avg", False, False, None)
            assert torch.equal(e["x0"], a["x0"]) and torch.equal(e["key_pad"], F._c(ref["key_pad"]).to(DEV)), tag
            eb, _ = ex_bwd(ops, c, g, ref, "avg", False, False, None)
            assert torch.equal(eb["d_modal"], ab["d_modal"]) and all(torch.equal(x, ab[f"du{i}"]) for i, x in enumerate(eb["du"])), tag
    RAN.update({("vct_mm_frontend_fwd", dtype), ("vct_mm_frontend_bwd", dtype)})
    report(capsys, "mm_frontend", worst)


# ---- vct_enc_frontend (single stream) -----------------------------------------------------------------------------------------------------------
@TYPES
def test_enc_frontend_single_stream(ops, dtype, capsys):
    worst = 0.0
    for tag, c in F.single_cases(dtype):
        g = Dev(c)
        B, T, d = c.B, c.Ts[0], c.d
        ref = F.reference(c, "avg", False, False)

        def fwd():
            a = Arena([mat("z", B * (T + 1), d, dtype)])
            ops.enc_frontend_fwd(g.us[0], g.temp, a["z"], B, T)
            return a

        def bwd():
            a = Arena([mat("du", B * T, d, dtype)])
            ops.enc_frontend_bwd(g.dx, a["du"], B, T)
            return a
        worst = max(worst, F.judge(f"single {tag} fwd", dict(x0=twice(fwd)["z"]), ref, c, "avg", False))
        worst = max(worst, F.judge(f"single {tag} bwd", dict(du=[twice(bwd)["du"]]), ref, c, "avg", False))
    RAN.update({("vct_enc_frontend_fwd", dtype), ("vct_enc_frontend_bwd", dtype)})
    report(capsys, "enc_frontend", worst)


# ---- vct_hmm_mix ----------------------------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


@TYPES
def test_hmm_mix(ops, dtype, capsys):
    worst = 0.0
    for B, S, d in Z["mix"][dtype]:
        M = B * S
        takes = [torch.zeros(S, dtype=U8), torch.ones(S, dtype=U8), (torch.arange(S) % 2).to(U8)]
        y, x0 = F.rnd((M, d), 61, 1.0, dtype), F.rnd((M, d), 62, 1.0, dtype)
        dxs = [F.rnd((M, d), 63 + k, 1.0, dtype) for k in range(3)]
        yg, x0g, dxg = guard(y), guard(x0), [guard(t) for t in dxs]
        for take in takes:
            tg = take.to(DEV)

            def fwd():
                a = Arena([mat("x", M, d, dtype)])
                ops.hmm_mix_fwd(yg, x0g, tg, a["x"], B, S)
                return a
            assert torch.equal(twice(fwd)["x"].cpu(), F.mix_fwd(y, x0, take, B, S))
            cont = take.bool().repeat(B)
            acc0 = F.rnd((M, d), 70)

            def bwd(init):
                def build():
                    a = Arena([mat("dy", M, d, dtype), mat("acc", M, d, F32)])
                    if not init:
                        a["acc"][~cont.to(DEV)] = acc0.to(DEV)[~cont.to(DEV)]      # the continuing rows keep the arena's 0xFF
                    ops.hmm_mix_bwd(dxg[0], tg, a["acc"], B, S, dy=a["dy"], init=init)
                    return a
                return twice(build, nonfinite_ok=() if init else ("acc",))
            for init in (True, False):
                a = bwd(init)
                dy, acc = F.mix_bwd(dxs[0], take, acc0, B, S, init=init)
                assert torch.equal(_bits(a["dy"].cpu()), _bits(dy)), "dy (restarting rows: +0 bit for bit)"
                got = a["acc"].cpu()
                assert torch.equal(_bits(got[~cont]), _bits(acc[~cont]))
                if init:
                    assert bool((_bits(got[cont]) == 0).all()), "acc: +0 on the continuing rows with init"
                else:
                    assert bool((got[cont].contiguous().view(U8) == 0xFF).all()), "acc: continuing rows touched without init"
        # a three-layer chain, top layer first: init, accumulate, close
        order = [takes[2], (1 - takes[2]), None]
        tgs = [t.to(DEV) for t in order[:2]]

        def chain():
            a = Arena([mat("dy0", M, d, dtype), mat("dy1", M, d, dtype), mat("acc", M, d, F32), mat("dx0", M, d, dtype)])
            ops.hmm_mix_bwd(dxg[0], tgs[0], a["acc"], B, S, dy=a["dy0"], init=True)
            ops.hmm_mix_bwd(dxg[1], tgs[1], a["acc"], B, S, dy=a["dy1"])
            ops.hmm_mix_bwd(dxg[2], None, a["acc"], B, S, dx0=a["dx0"])
            return a
        a = twice(chain)
        _, acc = F.mix_bwd(dxs[0], order[0], None, B, S, init=True)
        _, acc = F.mix_bwd(dxs[1], order[1], acc, B, S)
        assert torch.equal(_bits(a["acc"].cpu()), _bits(acc)), "acc after the chain (the closing form must not write it)"
        v, e = F.mix_close(dxs[2], acc)
        worst = max(worst, F.check_elem(f"mix dx0 {B}x{S}x{d}", a["dx0"].cpu(), v, F.R.bound(v, e, dtype)))
    RAN.update({("vct_hmm_mix_fwd", dtype), ("vct_hmm_mix_bwd", dtype)})
    report(capsys, "hmm_mix dx0", worst)


# ---- vct_gather_pad_rows ------------------------------------------------------------------------------------------------------------------------------
@TYPES
def test_gather_pad_rows(ops, dtype):
    from vct_amd import _lib as L
    lib = L.load()
    for E in Z["gather_E"]:
        for B, Tmax in Z["gather_BT"]:
            for zero in ("none", "middle", "last"):
                store, offs, idx = F.gather_case(E, B, Tmax, seed=E + B, zero=zero)
                if zero == "last":
                    assert int(offs[int(idx[-1])]) == store.shape[0]
                sg, og, ig = guard(store, extra=Tmax + 2), offs.to(DEV), idx.to(DEV)

                def build():
                    a = Arena([mat("out", B * Tmax, E, dtype), mat("mask", B, Tmax, U8)])
                    L.check(lib.vct_gather_pad_rows(L.dtype_code(dtype), B, Tmax, E, sg.data_ptr(), og.data_ptr(), ig.data_ptr(),
                                                    a["out"].data_ptr(), a["mask"].data_ptr(), L.stream_ptr()), "vct_gather_pad_rows")
                    return a
                a = twice(build)
                ref, mask = F.gather_pad(store, offs, idx, Tmax)
                what = f"gather E={E} B={B} Tmax={Tmax} zero={zero}"
                assert torch.equal(a["mask"].cpu(), mask), what + ": mask bytes"
                ref32 = ref.view(B * Tmax, E).to(F32)
                if dtype == F32:
                    F.check_bits(what, F.f32_bits(a["out"]), F.f32_bits(ref32))
                else:
                    F.check_bits(what, F.bf_bits(a["out"]), F.cast_rne(F.f32_bits(ref32)))
    RAN.add(("vct_gather_pad_rows", dtype))


# ---- vct_cast ---------------------------------------------------------------------------------------------------------------------------------------------
def _cast(ops, src, dst_dtype):
    n = src.numel()
    sg = src.to(DEV)

    def build():
        a = Arena([mat("dst", 1, n, dst_dtype)])
        ops.cast(sg, a["dst"])
        return a
    return twice(build, nonfinite_ok=("dst",))["dst"].view(-1)


def test_cast_rounding_over_the_pattern_set(ops):
    pat = F.cast_patterns()
    got = F.bf_bits(_cast(ops, F.bits_f32(pat), BF))
    F.check_bits("cast fp32 -> bf16", got, F.cast_rne(pat), nan_class=True)
    all16 = np.arange(65536, dtype=np.uint16)
    wide = F.f32_bits(_cast(ops, F.bits_bf(all16), F32))
    F.check_bits("cast bf16 -> fp32", wide, all16.astype(np.uint32) << 16)
    F.check_bits("cast bf16 -> bf16", F.bf_bits(_cast(ops, F.bits_bf(all16), BF)), all16)
    F.check_bits("cast fp32 -> fp32", F.f32_bits(_cast(ops, F.bits_f32(pat), F32)), pat)
    RAN.update({("vct_cast", F32), ("vct_cast", BF)})


@pytest.mark.parametrize("src,dst", [(F32, BF), (BF, F32), (F32, F32), (BF, BF)], ids=["f32-bf16", "bf16-f32", "f32-f32", "bf16-bf16"])
def test_cast_lengths(ops, src, dst):
    for n in Z["cast_n"]:
        x = F.rnd((n,), 80 + n % 97, 3.0, src)
        got = _cast(ops, x, dst).cpu()
        if src == F32 and dst == BF:
            F.check_bits(f"cast n={n}", F.bf_bits(got), F.cast_rne(F.f32_bits(x)))
        else:
            assert torch.equal(got, x.to(dst)), n


# ---- vct_transpose ----------------------------------------------------------------------------------------------------------------------------------------
def test_transpose(ops):
    for rows, cols in Z["transpose"]:
        pat = ((np.arange(rows * cols, dtype=np.uint32) * 40503 + 0x7F00) & 0xFFFF).astype(np.uint16)     # NaN patterns among them
        src = F.bits_bf(pat).view(rows, cols)
        want = F.bf_bits(F.transpose(src))
        odd = lambda x: x + 1 if x % 2 == 0 else x + 2
        # (ld_src, ld_dst, skew of dst): the vector path (both rounded up to 8), the element-wise path through odd leading dimensions
        # and through a base skewed by one element
        for lds, ldd, skew in ((up(cols, 8), up(rows, 8), 0), (odd(cols), odd(rows), 0), (up(cols, 8), up(rows, 8), 1)):
            sbuf = torch.full((rows, lds), NAN, dtype=BF, device=DEV)
            sbuf[:, :cols] = src.to(DEV)

            def build():
                a = Arena([mat("dst", cols, rows, BF, ldd, skew)])
                ops.transpose(sbuf[:, :cols], a["dst"])
                return a
            a = twice(build, nonfinite_ok=("dst",))
            F.check_bits(f"transpose {rows}x{cols} ld {lds}/{ldd} skew {skew}", F.bf_bits(a["dst"].contiguous()), want)
    RAN.add(("vct_transpose", BF))


# ---- coverage -------------------------------------------------------------------------------------------------------------------------------------------------
def test_every_entry_point_ran_in_every_type(ops):
    missing = [(k, t) for k, n in ENTRY_POINTS.items() for t in ((F32, BF) if n == 2 else (BF,)) if (k, t) not in RAN]
    assert not missing, f"entry points no case of this file judged: {missing}"
