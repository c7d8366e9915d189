"""The CLIP text tower on the GPU (vct_amd.text.ClipTextTower; csrc/vct_text.hip; VCT_ACT_QUICK_GELU), against the fp64 restatement
tests/text_tower_ref.py (itself held to transformers' module by tests/test_text_tower_cpu.py).

Harness, in the manner of tests/test_decode_block_gpu.py: every kernel output lies between canary rows, everything a kernel must not
read is NaN, every launch runs twice and must give the same bits.

Bounds (none sized from the kernels under test; u = 2^-8 for a bf16 result, 2^-24 for an fp32 one, the unit roundoff):
  LayerNorm kernels   fp32 arithmetic on a given row: |y - ref| <= u |ref| + 2e-5 max|ref| per element (2e-5: TOL[float32] of
                      tests/test_kernels_gpu.py, here applied to the largest element instead of the norm).  A CONSTANT row c: the exact
                      answer is beta; the kernel's mean carries at most 24 fp32 roundings (16 adds in a lane, 6 shuffle levels, the
                      division, the subtraction), the variance is then ~0 and rstd <= 1 / sqrt(1e-5), so
                      |y - beta| <= |gamma| 24 2^-24 |c| / sqrt(1e-5) (1 + u) + u |beta|.
  GEMM with QuickGELU tests/gemm_ref.py's formula with this activation's constants: |got - ref| <= u |ref| + 1.1 acc_term + 2^-20 |q(z)|
                      (1 + |z|), acc_term = (K + 1) 2^-24 (S + |bias|).  max |q'| = 1.0998 at z = 1.41; the activation itself is one
                      multiply, v_exp (1 ulp) of an argument rounded once -- a relative error of 1.702 |z| 2^-24 in the exponential --
                      one add, v_rcp (1 ulp), one multiply: below (5 + 1.702 |z|) 2^-24 |q(z)| < 2^-20 (1 + |z|) |q(z)| (fp32 kernel:
                      expf and a division, tighter).
  stages of the tower each stored intermediate against fp64 of the SAME operation on the operand stored one stage earlier: the
                      LayerNorm bound, the GEMM bound (plus u |addend| where the stream is added), and for the attention core the
                      relative-Frobenius figures of tests/test_attention_kernels_gpu.py, 2e-5 (fp32) / 1.5e-2 (bf16).
  end to end          relative Frobenius against the exact restatement: 1e-3 (fp32), 3e-2 (bf16) -- SURVEY 8(d)."""
import math

import pytest
import torch

import gemm_ref as G
import matching_ref as MR
import text_tower_ref as R
from helpers import GradTol, build_model, load_golden

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
CANARY = -776.0          # exact in bf16 and int32
NAN = float("nan")
U = {BF: 2.0 ** -8, F32: 2.0 ** -24}
DT = [pytest.param(F32, id="fp32"), pytest.param(BF, id="bf16")]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from vct_amd import ops as _ops
    return _ops


def rnd(*shape, seed, scale=1.0, dtype=F32):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(DEV)


def d64(t):
    return t.detach().to(F64)


class Guard:
    """`n` rows of `cols` for a kernel to write, inside a canary-filled buffer (one row in front, two behind)."""

    def __init__(self, n, cols, dtype=F32):
        self.n, self.buf = n, torch.empty(n + 3, cols, dtype=dtype, device=DEV)
        self.reset()

    def reset(self):
        self.buf.fill_(CANARY)

    @property
    def view(self):
        return self.buf[1:1 + self.n]

    def intact(self):
        return bool((self.buf[0] == CANARY).all()) and bool((self.buf[1 + self.n:] == CANARY).all())


def twice(launch, guards):
    """launch() on fresh canaries, twice: finite, bit-identical outputs and intact canaries."""
    launch()
    first = [g.view.clone() for g in guards]
    for g in guards:
        g.reset()
    launch()
    torch.cuda.synchronize()
    for a, g in zip(first, guards):
        assert g.intact(), "a canary row was overwritten"
        assert bool(torch.isfinite(g.view.float()).all()), "NaN / Inf / canary left in an output"
        assert bool((g.view != CANARY).all()), "an output element was not written"
        assert torch.equal(a, g.view), "a second identical call gave different bits"


def check_elem(what, got, ref, bnd):
    excess = torch.nan_to_num(((d64(got) - ref).abs() - bnd), nan=float("inf"))
    worst = float(excess.max())
    print(f"[text-tower] {what}: worst |got - ref| - bound = {worst:.3e}; max |got - ref| = {float((d64(got) - ref).abs().max()):.3e}")
    assert worst <= 0.0, (what, worst)


def relf(got, ref):
    return float((d64(got) - ref).norm() / ref.norm().clamp_min(1e-30))


def ln_bound(ref, dtype):
    return U[dtype] * ref.abs() + 2e-5 * ref.abs().max()


# ---- vct_preln_fwd ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("d", [64, 72, 512, 1024])
def test_preln_fwd(ops, d, dtype):
    gam, bet = 1 + 0.2 * rnd(d, seed=d + 1), 0.3 * rnd(d, seed=d + 2)
    for M in (1, 5, 257):
        # NaN rows around the M the kernel may read; row 0 (M >= 5: also row 3) is constant
        xb = torch.full((M + 2, d), NAN, device=DEV)
        x = xb[1:1 + M]
        x.copy_(rnd(M, d, seed=M * 7 + d, scale=1.5) + 0.7)
        const = [0] if M == 1 else [0, 3]
        for i, r in enumerate(const):
            x[r] = (3.0, -0.37)[i]
        y = Guard(M, d, dtype)
        twice(lambda: ops.preln_fwd(x, gam, bet, y.view), [y])
        ref = R.layer_norm(d64(x), d64(gam), d64(bet))
        keep = torch.ones(M, dtype=torch.bool, device=DEV)
        keep[const] = False
        check_elem(f"preln d={d} M={M} {dtype}", y.view[keep], ref[keep], ln_bound(ref[keep], dtype)) if keep.any() else None
        for r in const:
            c = float(x[r, 0].abs())
            bnd = d64(gam).abs() * 24 * 2.0 ** -24 * c / math.sqrt(1e-5) * (1 + U[dtype]) + U[dtype] * d64(bet).abs() + 1e-30
            check_elem(f"preln constant row {c} d={d} M={M} {dtype}", y.view[r], d64(bet), bnd)


# ---- vct_text_pool ---------------------------------------------------------------------------------------------------------------------------
def pool_case(B, L, width, vocab, seed):
    """ids [B, width] whose first maxima lie at 1, L - 1, a repeated maximum (first copy wins), and random places."""
    g = torch.Generator().manual_seed(seed)
    e = [1, L - 1, max(1, L // 2)] + torch.randint(1, L, (max(B - 3, 0),), generator=g).tolist()
    e = e[:B]
    ids = R.caption_ids(e, vocab, seed, width=width)
    if B >= 3 and e[2] + 1 < width:
        ids[2, e[2] + 1:] = torch.where(torch.rand(width - e[2] - 1, generator=g) < 0.5, vocab - 1, 0)      # EOT again, behind
        ids[2, width - 1] = vocab - 1
    return ids, e


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("d", [64, 72, 512, 1024])
def test_text_pool(ops, d, dtype):
    gam, bet = 1 + 0.2 * rnd(d, seed=d + 3), 0.3 * rnd(d, seed=d + 4)
    for B, L, width in ((1, 2, 2), (5, 9, 77), (257, 64, 64), (6, 64, 77)):
        ids, e = pool_case(B, L, width, 1000, seed=B + d)
        assert R.first_argmax(ids).tolist() == e
        # the stream: NaN everywhere but the B rows the kernel has to gather
        x = torch.full((B * L, d), NAN, device=DEV)
        rows = torch.tensor([b * L + e[b] for b in range(B)], device=DEV)
        x[rows] = rnd(B, d, seed=B * 3 + d, scale=2.0) - 0.4
        ids_dev = torch.full((B + 1, width + 3), -5, dtype=torch.int64, device=DEV)[:B, :width]      # a strided view: ld_ids > width
        ids_dev.copy_(ids)
        y, eot = Guard(B, d, dtype), Guard(1, B, torch.int32)
        err = torch.zeros(1, dtype=torch.int32, device=DEV)
        twice(lambda: ops.text_pool(ids_dev, x, L, gam, bet, y.view, eot.view[0], err), [y, eot])
        assert eot.view[0].tolist() == e and int(err) == 0
        ref = R.layer_norm(d64(x[rows]), d64(gam), d64(bet))
        check_elem(f"text_pool d={d} B={B} L={L} {dtype}", y.view, ref, ln_bound(ref, dtype))


def test_text_pool_flags_a_row_behind_the_trim(ops):
    """Only the first L = 8 positions were run but caption 1 ends at 11: the flag rises, that row is zero, the others are right."""
    d, L, width = 64, 8, 16
    ids = R.caption_ids((3, 11, 7), 500, seed=1, width=width)
    x = rnd(3 * L, d, seed=2)
    gam, bet = 1 + 0.2 * rnd(d, seed=3), 0.3 * rnd(d, seed=4)
    y, eot = Guard(3, d, F32), Guard(1, 3, torch.int32)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    twice(lambda: ops.text_pool(ids.to(DEV), x, L, gam, bet, y.view, eot.view[0], err), [y, eot])
    assert eot.view[0].tolist() == [3, 11, 7] and int(err) == 1
    assert bool((y.view[1] == 0).all())
    ref = R.layer_norm(d64(x[[3, 2 * L + 7]]), d64(gam), d64(bet))
    check_elem("text_pool beside a flagged row", y.view[[0, 2]], ref, ln_bound(ref, F32))


# ---- QuickGELU on every GEMM route that carries an activation -----------------------------------------------------------------------------------
QG_CASES = [
    # name, route, dtype, out, (M, N, K), tile, ldc
    ("general-bf16-vector", dict(kernel=1, bm=64, bn=64), BF, BF, (65, 72, 72), 4, None),
    ("general-bf16-scalar", dict(kernel=1, bm=64, bn=64), BF, F32, (63, 77, 200), 4, 77),
    ("general-bf16-128", dict(kernel=1, bm=128, bn=128), BF, BF, (129, 127, 64), 5, 127),
    ("fp32", dict(kernel=2, bm=64, bn=64), F32, F32, (65, 63, 20), 0, None),
    ("fp32-ragged-k", dict(kernel=2, bm=64, bn=64), F32, F32, (63, 65, 52), 0, None),
    ("skinny-bf16", dict(kernel=3), BF, BF, (17, 17, 72), 0, 24),
    ("skinny-fp32-out", dict(kernel=3), BF, F32, (1, 16, 64), 0, None),
    ("layer-64", dict(kernel=6, bm=64, bn=128, variant=1), BF, BF, (1025, 256, 136), 100, None),
    ("layer-128", dict(kernel=6, bm=128, bn=128, variant=1), BF, BF, (1024, 1032, 128), 0, None),
]


@pytest.mark.parametrize("case", QG_CASES, ids=[c[0] for c in QG_CASES])
def test_quick_gelu_on_each_gemm_route(ops, case):
    name, route, dt, out, (M, N, K), tile, ldc = case
    a = G.rnd((M, K), 11, 1.0, dt, DEV)
    b = G.rnd((N, K), 12, 2.0 / math.sqrt(K), dt, DEV)             # z ~ N(0, 2^2): both tails of the activation
    bias = G.rnd((N,), 13, 0.5, F32, DEV)
    ldc = N if ldc is None else ldc
    c = Guard(M, ldc, out)

    def launch():
        ops.gemm(a, b, c.view[:, :N], bias=bias, act="quick_gelu", tile=tile)
    launch()
    first = c.view.clone()
    got_route = ops.gemm_last_route()
    assert all(got_route[k] == v for k, v in route.items()), (name, got_route)
    c.reset()
    launch()
    torch.cuda.synchronize()
    assert c.intact() and bool((c.view[:, N:] == CANARY).all()), "canary rows / padding columns written"
    assert torch.equal(first, c.view) and bool(torch.isfinite(c.view.float()).all())
    Z, S = G.product(a, b)
    z = Z + d64(bias)
    ref = R.quick_gelu(z)
    acc = (K + 1) * G.U24 * (S + d64(bias).abs())
    bnd = U[out] * ref.abs() + 1.1 * acc + G.U20 * ref.abs() * (1 + z.abs())
    check_elem(f"quick_gelu {name}", c.view[:, :N], ref, bnd)
    if z.numel() >= 1000:
        assert float(z.min()) < -3 and float(z.max()) > 3, "the operands no longer reach both tails of the activation"


def test_quick_gelu_has_no_derivative_form(ops):
    a, b = rnd(16, 64, seed=1, dtype=BF), rnd(64, 64, seed=2, dtype=BF)
    with pytest.raises(ValueError, match="VCT_E_ARG"):
        ops.gemm(a, b, torch.empty(16, 64, dtype=BF, device=DEV), tb=False, act="quick_gelu", dact_src=torch.zeros(16, 64, dtype=BF, device=DEV))


# ---- the tower ---------------------------------------------------------------------------------------------------------------------------------
TOWERS = {
    # name: (W, heads, ff, layers, P, vocab, std, EOT indices)
    "w64-L64": (64, 4, 256, 2, 48, 300, 0.1, (3, 9, 20, 63, 12)),
    "w72-hd24": (72, 3, 144, 2, 40, 300, 0.1, (5, 17, 2, 30)),
    "b1-L2": (64, 4, 256, 2, 48, 300, 0.1, (1,)),
    "w512": (512, 8, 2048, 2, 512, 1000, 0.06, (3, 9, 20, 31, 12, 7, 15, 5)),
}
_CACHE = {}


def case(name):
    """(state dict, ids [B, 77], exact fp64 features, heads), computed once per shape."""
    if name not in _CACHE:
        W, H, ff, nl, P, V, std, eots = TOWERS[name]
        sd = R.random_state_dict(W, H, ff, nl, P, V, seed=len(name) + W, std=std)
        ids = R.caption_ids(eots, V, seed=W + 1)
        _CACHE[name] = (sd, ids, R.tower(sd, ids, H, L=max(eots) + 1), H)
    return _CACHE[name]


def gemm_bound(ref, x, w, bias, dtype_out, addend=None, act=False):
    """tests/gemm_ref.py's bound for ref = epilogue(x @ w^T + bias) [+ addend], from fp64 copies of the operands as stored."""
    K = x.shape[1]
    acc = (K + 1) * G.U24 * (x.abs() @ w.abs().t() + bias.abs())
    b = U[dtype_out] * ref.abs() + (1.1 if act else 1.0) * acc
    if act:
        z = x @ w.t() + bias
        b = b + G.U20 * R.quick_gelu(z).abs() * (1 + z.abs())
    if addend is not None:
        b = b + U[dtype_out] * addend.abs()
    return b


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("name", list(TOWERS))
def test_tower_stage_by_stage(ops, name, dtype):
    from vct_amd.text import ClipTextTower
    sd, ids, _exact, H = case(name)
    t = ClipTextTower.from_state_dict(sd, DEV, dtype, heads=H)
    out = t.encode_ids(ids, keep=True)
    k = t.kept
    torch.cuda.synchronize()
    B, L = ids.shape[0], k["L"]
    assert L == max(TOWERS[name][7]) + 1 and k["eot"].tolist() == list(TOWERS[name][7]) and int(t.err) == 0
    t.check()
    x0 = d64(t.tok)[ids[:, :L].to(DEV)].reshape(B * L, -1) + d64(t.pos)[:L].repeat(B, 1)
    check_elem(f"{name} embedding", k["x0"], x0, U[F32] * x0.abs())
    x = d64(k["x0"])
    for li, (kl, lw) in enumerate(zip(k["layers"], t.lw)):
        w = {n: d64(v) for n, v in lw.items()}
        tag = f"{name} {dtype} layer {li}"
        ref = R.layer_norm(x, w["ln1_g"], w["ln1_b"])
        check_elem(f"{tag} ln_1", kl["h1"], ref, ln_bound(ref, dtype))
        h1 = d64(kl["h1"])
        ref = h1 @ w["w_qkv"].t() + w["b_qkv"]
        check_elem(f"{tag} qkv", kl["qkv"], ref, gemm_bound(ref, h1, w["w_qkv"], w["b_qkv"], dtype))
        ref = R.attention(d64(kl["qkv"]), B, L, H)
        e = relf(kl["o"], ref)
        print(f"[text-tower] {tag} attention: rel-Frobenius {e:.3e}")
        assert e <= (1.5e-2 if dtype == BF else 2e-5)
        o = d64(kl["o"])
        ref = x + o @ w["w_o"].t() + w["b_o"]
        check_elem(f"{tag} out_proj + stream", kl["x1"], ref, gemm_bound(ref, o, w["w_o"], w["b_o"], F32, addend=x))
        x1 = d64(kl["x1"])
        ref = R.layer_norm(x1, w["ln2_g"], w["ln2_b"])
        check_elem(f"{tag} ln_2", kl["h2"], ref, ln_bound(ref, dtype))
        h2 = d64(kl["h2"])
        ref = R.quick_gelu(h2 @ w["w_fc"].t() + w["b_fc"])
        check_elem(f"{tag} c_fc + QuickGELU", kl["f"], ref, gemm_bound(ref, h2, w["w_fc"], w["b_fc"], dtype, act=True))
        f = d64(kl["f"])
        ref = x1 + f @ w["w_proj"].t() + w["b_proj"]
        check_elem(f"{tag} c_proj + stream", kl["x2"], ref, gemm_bound(ref, f, w["w_proj"], w["b_proj"], F32, addend=x1))
        x = d64(kl["x2"])
    rows = x.reshape(B, L, -1)[torch.arange(B, device=DEV), k["eot"].long()]
    ref = R.layer_norm(rows, d64(t.lnf_g), d64(t.lnf_b))
    check_elem(f"{name} {dtype} ln_final of the EOT rows", k["pooled"], ref, ln_bound(ref, dtype))
    pooled, proj = d64(k["pooled"]), d64(t.proj)
    ref = pooled @ proj.t()
    check_elem(f"{name} {dtype} projection", out, ref, gemm_bound(ref, pooled, proj, torch.zeros(proj.shape[0], dtype=F64, device=DEV), F32))
    assert torch.equal(out, k["out"]) and out.dtype == F32 and tuple(out.shape) == (B, t.dim)
    assert torch.equal(t.encode_ids(ids), out), "a second identical call gave different bits"


@pytest.mark.parametrize("dtype", DT)
def test_end_to_end_against_the_exact_restatement(ops, dtype):
    from vct_amd.text import ClipTextTower
    bound = 1e-3 if dtype == F32 else 3e-2
    tol = GradTol("text_tower_end_to_end", dtype, bound)
    for name in TOWERS:
        sd, ids, exact, H = case(name)
        t = ClipTextTower.from_state_dict(sd, DEV, dtype, heads=H)
        tol.add(name, relf(t.encode_ids(ids), exact.to(DEV)))
    # the recorded transformers model (3 layers; tests/golden/text_tower.npz), from transformers' key convention
    z = load_golden("text_tower.npz")
    sd = {k[2:]: torch.from_numpy(z[k]).to(F64) * float(z["scale/" + k[2:]]) for k in z.files if k.startswith("q/")}
    t = ClipTextTower.from_state_dict(sd, DEV, dtype, heads=int(z["heads"]))
    got = t.encode_ids(torch.from_numpy(z["ids"]))
    tol.add("golden-transformers", relf(got, torch.from_numpy(z["out"]).to(DEV)))
    t.check()
    print("[text-tower] end to end:", tol.errs)
    tol.report()


@pytest.mark.parametrize("dtype", DT)
def test_trimmed_against_untrimmed_and_every_input_form(ops, dtype):
    """The same captions padded to 40 and to 64 columns (and to CLIP's 77): host ids are trimmed to the same L, so the features are
    bit-identical; int32 ids too; encode_all in chunks (each trimmed to its own L) and device-resident ids (run untrimmed) agree with
    them to the end-to-end bound's scale."""
    from vct_amd.text import ClipTextTower
    sd, _ids, _exact, H = case("w64-L64")
    t = ClipTextTower.from_state_dict(sd, DEV, dtype, heads=H)
    eots = (3, 9, 20, 33, 12, 5, 2)
    ids77 = R.caption_ids(eots, 300, seed=9)
    a40, a64, a77 = t.encode_ids(ids77[:, :40]), t.encode_ids(ids77[:, :64]), t.encode_ids(ids77)
    assert torch.equal(a40, a64) and torch.equal(a40, a77) and torch.equal(a40, t.encode_ids(ids77[:, :40].to(torch.int32)))
    exact = R.tower(sd, ids77, H, L=34).to(DEV)
    bound = 1e-3 if dtype == F32 else 3e-2
    assert relf(a40, exact) <= bound
    allc = Guard(len(eots), t.dim)
    t.encode_all(ids77, chunk=3, out=allc.view)
    on_dev = t.encode_ids(ids77[:, :40].to(DEV))
    torch.cuda.synchronize()
    assert allc.intact() and relf(allc.view, exact) <= bound and relf(on_dev, exact) <= bound
    t.check()
    assert set(t._bufs) >= {(7, 34), (3, 21), (3, 34), (1, 3), (7, 40)}            # buffers per (B, L)
    # device ids whose EOT lies behind the 64 positions that can be run: the lazy flag, not a wrong row
    far = R.caption_ids((3, 70), 300, seed=1).to(DEV)
    t.encode_ids(far)
    with pytest.raises(ValueError, match="behind position 64"):
        t.check()
    t.check()                                                                        # read once, cleared


def test_tower_is_recorded_by_a_launch_list(ops):
    """Every launch of the forward goes through the runtime's wrapper: a launch list records 7 per layer + 3 and replays them."""
    from vct_amd.text import ClipTextTower
    sd, ids, _exact, H = case("w64-L64")
    t = ClipTextTower.from_state_dict(sd, DEV, BF, heads=H)
    ids_dev = ids[:, :64].to(DEV)
    want = t.encode_ids(ids_dev).clone()
    out = torch.zeros_like(want)
    ll = ops.LaunchList()
    with ll.record():
        t.encode_ids(ids_dev, out=out)
    assert len(ll) == 7 * t.layers + 3, len(ll)
    out.zero_()
    ll.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    ll.close()


# ---- integration: the matching task with the tower installed -------------------------------------------------------------------------------------
V = 131


def clip_like_tokenize(captions):
    """Stand-in for clip.tokenize (no BPE here): id rows of the model's vocabulary, or strings, -> int64 [B, 77] with a start token,
    one id per word and the EOT (the largest id, 299) behind them."""
    rows = []
    for c in captions:
        words = [int(v) % 290 + 1 for v in c.tolist() if int(v) != 0] if torch.is_tensor(c) else [sum(map(ord, w)) % 290 + 1 for w in c.split()]
        rows.append([298] + words[:60] + [299])
    ids = torch.zeros(len(rows), 77, dtype=torch.int64)
    for b, r in enumerate(rows):
        ids[b, :len(r)] = torch.tensor(r)
    return ids


def match_model(dtype, seed=5):
    mc = MR.matching_config([48], 48, MR.matching_block("CSL", "fixed", 0.5))
    return build_model(mc, V, DEV, dtype, MR.matching_params(mc, V, seed))


@pytest.mark.parametrize("task", ["match", "cross"])
def test_trainer_step_with_the_tower_installed(ops, task):
    """CaptionTrainer.step with captions and an installed tower == the same step with text_feats=tower(captions), bit for bit."""
    from mm_ref import mm_batch
    from vct_amd.text import ClipTextTower
    from vct_amd.trainer import CaptionTrainer
    sd, _ids, _exact, H = case("w64-L64")
    feats, masks, ids = mm_batch(4, (5,), (48,), 7, V, seed=9)
    f, mk, ids = torch.from_numpy(feats[0]).to(DEV), torch.from_numpy(masks[0]).to(DEV), torch.from_numpy(ids).to(DEV)
    losses = []
    for installed in (True, False):
        m = match_model(F32)
        tower = ClipTextTower.from_state_dict(sd, DEV, F32, tokenize=clip_like_tokenize, heads=H)
        assert m.text_encoder.backend is None
        if installed:
            m.install_text_encoder(tower)
        m.mode(task)
        m.train()
        tr = CaptionTrainer(m, torch.optim.Adam([m.flat_params], lr=1e-4))
        out = tr.step(f, mk, ids) if installed else tr.step(f, mk, ids, tower(ids))
        out = out if isinstance(out, tuple) else (out,)
        losses.append([float(o.reshape(-1)[0]) for o in out])
        assert not any(n.startswith("text") for n in m.state_dict())
        tower.check()
    assert losses[0] == losses[1] and all(math.isfinite(v) for v in losses[0]), losses
    # the model's own forward takes the captions too
    m = match_model(F32)
    tower = m.install_text_encoder(ClipTextTower.from_state_dict(sd, DEV, F32, tokenize=clip_like_tokenize, heads=H))
    m.mode(task)
    m.eval()
    with torch.no_grad():
        a, b = m([f], [mk], ids), m([f], [mk], ids, text_feats=tower(ids))
    a, b = (a if isinstance(a, tuple) else (a,)), (b if isinstance(b, tuple) else (b,))
    assert all(torch.equal(p, q) for p, q in zip(a, b))


def test_eval_retrieval_with_the_tower_installed(ops):
    """eval_retrieval over a 12-caption split: the installed tower (strings through its tokenizer) gives the dict that
    text_feats_fn=tower gives."""
    from mm_ref import mm_batch
    from vct_amd import evaluate
    from vct_amd.text import ClipTextTower
    sd, _ids, _exact, H = case("w64-L64")
    m = match_model(F32)
    tower = ClipTextTower.from_state_dict(sd, DEV, F32, tokenize=clip_like_tokenize, heads=H)
    feats, masks, _ = mm_batch(6, (5,), (48,), 7, V, seed=3)
    f, mk = torch.from_numpy(feats[0]), torch.from_numpy(masks[0])
    vids = [f"video{k}" for k in range(6)]
    words = "a man is cooking the dog runs on grass two people talk about cars".split()
    v2c = {v: [" ".join(words[(k + 3 * j + i) % len(words)] for i in range(3 + j + k)) for j in range(2)] for k, v in enumerate(vids)}
    assert sum(map(len, v2c.values())) == 12

    class Split:
        dataset = type("D", (), {"video2caption": v2c})()

        def __iter__(self):
            return iter([([f[:3]], [mk[:3]], None, vids[:3]), ([f[3:]], [mk[3:]], None, vids[3:])])
    m.mode("match")
    with pytest.raises(RuntimeError, match="no text encoder"):
        evaluate.eval_retrieval(m, Split())
    want = evaluate.eval_retrieval(m, Split(), text_feats_fn=lambda caps, _v: tower(caps))
    m.install_text_encoder(tower)
    got = evaluate.eval_retrieval(m, Split())
    assert got == want and got["t2v"]["n"] == 12 and got["v2t"]["n"] == 6
    tower.check()
