"""The gradient-clipping kernels alone (csrc/vct_grad_clip.hip) against the fp64 definition of tests/grad_clip_ref.py, on guarded
memory: NaN (0xFF bytes) in every gap between segments and around them, canaries around every buffer, every case run twice and
required to give the same bits.

Tolerances.  Small integers: every square and every partial sum is an integer below 2^53, so the fp64 sum is exact in any order
and norm must be fp32(sqrt(exact)) bit for bit.  Anything else: the device adds at most 2^21 exact fp64 products per case
(relative error below 2^21 * 2^-53 ~ 2.4e-10), takes one correctly rounded fp64 sqrt and rounds once to fp32 (half an ulp = 6e-8
relative): the result is the fp32 neighbour of the definition's at worst -> 1 ulp.  coef is checked as the fp32 formula on the
DEVICE's own norm, bit for bit (no fast-math: add and divide are correctly rounded), the scaled elements as fp32(g * coef) with
the coefficient read back, bit for bit."""
import numpy as np
import pytest
import torch

import grad_clip_ref as R
from gpu_arena import Arena

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _many(n=300, seed=5):
    """n segments of 4 .. 260 elements (more than the finishing workgroup has waves or threads), gaps of 0 .. 11 elements."""
    r = np.random.default_rng(seed)
    segs, at = [], 0
    for _ in range(n):
        k = int(r.integers(4, 261))
        segs.append((at, at + k))
        at = (at + k + int(r.integers(0, 9)) + 3) // 4 * 4
    return segs


LAYOUTS = {
    "one4": [(0, 4)],
    "4092": [(0, 4092)], "4096": [(0, 4096)], "4100": [(0, 4100)],
    "three": [(0, 7), (64, 64 + 4101), (8256, 8256 + 12)],
    "many300": _many(),
    "big": [(0, 2 ** 20 + 4)],                              # 257 partials
}
KINDS = ["ints", "normal", "zeros", "huge", "tiny", "one_nan", "one_inf"]
_cache = {}


def _case(layout, kind):
    """(flat fp32 with NaN bytes in every gap, segments, max_norm) -- built once per case and never modified."""
    key = (layout, kind)
    if key in _cache:
        return _cache[key]
    segs = LAYOUTS[layout]
    total = (segs[-1][1] + 3) // 4 * 4 + 8                  # a NaN tail behind the last segment too
    flat = np.full(total, 0xFFFFFFFF, np.uint32).view(F32)
    r = np.random.default_rng(sum(map(ord, layout + kind)))
    for a, b in segs:
        n = b - a
        if kind == "ints":
            v = r.integers(-8, 9, n).astype(F32)
        elif kind == "zeros":
            v = np.zeros(n, F32)
        elif kind == "huge":
            v = (F32(3e19) * r.choice([-1.0, 1.0], n)).astype(F32)
        elif kind == "tiny":
            v = (F32(1e-30) * r.uniform(0.5, 1.5, n)).astype(F32)
        else:
            v = r.standard_normal(n).astype(F32)
        flat[a:b] = v
    if kind in ("one_nan", "one_inf"):
        a, b = segs[len(segs) // 2]
        flat[a + (b - a) // 2] = F32(np.nan) if kind == "one_nan" else F32(-np.inf)
    ref_norm = R.norms(flat, segs)[0]
    max_norm = float(ref_norm) * 0.37 if np.isfinite(ref_norm) and ref_norm > 0 else 1.0
    flat.setflags(write=False)
    _cache[key] = (flat, segs, max_norm)
    return _cache[key]


def _run(flat, segs, max_norm=None, max_value=None):
    """One norm + apply (or one value clamp) on a fresh arena; everything read back as numpy."""
    from vct_amd import ops
    table = ops.grad_segments_table(segs, DEV)
    _, nseg, blocks = table
    A = Arena([("g", 1, flat.size, torch.float32, flat.size, 0), ("partials", 1, blocks + nseg, torch.float64, blocks + nseg, 0),
               ("seg_norm", 1, nseg, torch.float32, nseg, 0), ("state", 1, 4, torch.float32, 4, 0)])
    g = A["g"][0]
    g.copy_(torch.from_numpy(flat.copy()))
    clip = torch.tensor([max_norm or 0.0, max_value or 0.0], dtype=torch.float32, device=DEV)
    if max_value is None:
        ops.grad_sqnorm(g, table, A["partials"][0], A["seg_norm"][0], clip, A["state"][0])
        ops.grad_clip_apply(g, table, clip, A["state"][0], "norm")
    else:
        ops.grad_clip_apply(g, table, clip, None, "value")
    torch.cuda.synchronize()
    if max_value is None:
        A.check(nonfinite_ok=("g", "partials", "seg_norm", "state"))
    else:                                                    # the value mode writes none of the norm pass's outputs
        assert all(bool((A[k].contiguous().view(-1).view(torch.uint8) == 0xFF).all()) for k in ("partials", "seg_norm", "state"))
        for a, b in A.guards:
            assert bool((A.buf[a:b] == A.CANARY).all())
    return {k: A[k][0].cpu().numpy() for k in ("g", "partials", "seg_norm", "state")}


def _same(x, y):
    return all(np.array_equal(x[k].view(np.uint8), y[k].view(np.uint8)) for k in x)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_norm_and_scale(layout, kind):
    flat, segs, max_norm = _case(layout, kind)
    out = _run(flat, segs, max_norm)
    assert _same(out, _run(flat, segs, max_norm)), "two runs differ"
    norm, coef = out["state"][0], out["state"][1]
    assert out["state"][2] == 0.0 and out["state"][3] == 0.0
    ref_norm, ref_seg, exact = R.norms(flat, segs)
    print(f"[grad-clip] {layout}/{kind}: norm {norm!r} ref {ref_norm!r} coef {coef!r}")
    assert R.check(flat, out["g"], segs, norm, coef, out["seg_norm"], max_norm, norm_ulps=1) == []
    if kind == "ints":                                       # exact in any order: no ulp at all
        assert R.same_bits(norm, F32(np.sqrt(np.float64(exact)))) and R.same_bits(out["seg_norm"], ref_seg)
        assert coef < 1.0
    elif kind == "zeros":
        assert R.same_bits(norm, F32(0.0)) and R.same_bits(coef, F32(1.0)) and not out["seg_norm"].any()
        assert R.same_bits(out["g"], flat)
    elif kind in ("huge", "tiny"):
        assert np.isfinite(norm) and norm > 0 and coef < 1.0
    elif kind == "normal":
        assert coef < 1.0
    elif kind == "one_nan":
        assert np.isnan(norm) and np.isnan(coef) and np.isnan(R.coef_of(ref_norm, max_norm))
        assert int(np.isnan(out["seg_norm"]).sum()) == 1
    elif kind == "one_inf":
        assert np.isposinf(norm) and R.same_bits(coef, R.coef_of(ref_norm, max_norm)) and coef == 0.0


@pytest.mark.parametrize("max_norm", [1e30, float("inf")])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_inactive_clipping_touches_nothing(layout, max_norm):
    """coef == 1: the norm is measured and the whole buffer -- segments, gaps, tail -- keeps its bits."""
    flat, segs, _ = _case(layout, "normal")
    out = _run(flat, segs, max_norm)
    assert R.same_bits(out["state"][1], F32(1.0)) and R.same_bits(out["g"], flat)
    assert R.ulps(out["state"][0], R.norms(flat, segs)[0]) <= 1
    assert R.check(flat, out["g"], segs, out["state"][0], out["state"][1], out["seg_norm"], max_norm) == []


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_value_clamp(layout):
    """torch.clamp on the segments: NaN stays NaN, +-inf -> +-v, -0.0 is kept; the gaps keep their bits."""
    flat, segs, _ = _case(layout, "normal")
    flat = flat.copy()
    a, b = segs[-1]
    flat[a:a + 4] = np.array([np.nan, np.inf, -np.inf, -0.0], F32)
    v = 0.25
    out = _run(flat, segs, max_value=v)
    assert _same(out, _run(flat, segs, max_value=v)), "two runs differ"
    want = R.clip_by_value(flat, segs, v)
    got = out["g"]
    inside = np.zeros(flat.size, bool)
    for x, y in segs:
        inside[x:y] = True
    assert R.same_bits(got[~inside], flat[~inside])
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan) and R.same_bits(got[~nan], want[~nan])
    assert np.isnan(got[a]) and got[a + 1] == F32(v) and got[a + 2] == F32(-v) and got[a + 3] == 0.0 and np.signbit(got[a + 3])
    assert (np.abs(got[inside & ~nan]) <= F32(v)).all() and (np.abs(flat[inside & ~nan]) > F32(v)).any()
