"""The CLIP vision tower on the GPU (vct_amd.vision.ClipVisionTower; csrc/vct_vision.hip), against PIL, the lookup table and the fp64
restatement tests/vision_ref.py (itself held to PIL and to transformers' module by tests/test_vision_tower_cpu.py).

Every kernel output lies in a tests/gpu_arena.py arena (0xFF = NaN everywhere, canaries on both sides), everything a kernel must not
read is NaN, every launch runs twice and must give the same bits.

Bounds (none sized from the kernels under test; u = 2^-8 for a bf16 result, 2^-24 for an fp32 one):
  vct_frames_to_patches   none: the uint8 crop equals PIL's in every byte and the patch matrix equals lut[crop] in every bit.
  LayerNorm kernels       tests/test_text_tower_gpu.py's: |y - ref| <= u |ref| + 2e-5 max |ref| per element (vision_ref.ln_bound).
  stages of the tower     each stored intermediate against fp64 of the SAME operation on the operand stored one stage earlier:
                          tests/gemm_ref.py's GEMM bound (u |ref| + (K + 1) 2^-24 (|a| |b| + |bias|), 1.1 x and the 2^-20 |q(z)| (1 + |z|)
                          term with QuickGELU, u |addend| where the stream is added), the LayerNorm bound, and for the attention core the
                          relative-Frobenius figures of tests/test_attention_kernels_gpu.py, 2e-5 (fp32) / 1.5e-2 (bf16).
  end to end              relative Frobenius against the exact restatement: 1e-3 (fp32), 3e-2 (bf16), test_text_tower_gpu.py's."""
import numpy as np
import pytest
import torch

import gemm_ref as G
import text_tower_ref as TR
import vision_ref as R
from gpu_arena import Arena
from helpers import GradTol, load_golden

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
NAN = float("nan")
U = R.U
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


def relf(got, ref):
    return float((d64(got) - ref).norm() / ref.norm().clamp_min(1e-30))


# ---- vct_frames_to_patches -------------------------------------------------------------------------------------------------------------------
# the seven sizes of vision_ref.SIZES at (R, P) = (32, 16) -- down- and upscaling, identity, portrait, landscape, odd crop margins (20 x 31:
# 17 columns to cut, 8 on the left) -- one frame size at the real (224, 32), and two whose height is R already: both passes are skipped
# and only the crop remains, with an even (50 - 32) and an odd (45 - 32: 6 on the left, half to even) margin
F2P_CASES = [(H, W, 32, 16) for H, W, _R in R.SIZES] + [(240, 320, 224, 32), (32, 50, 32, 16), (32, 45, 32, 16)]


def f2p_frames(N, H, W, seed):
    """Random bytes; of three frames the last is pure 0 / 255 noise (the overshoot of the cubic runs into the clamp on both sides)."""
    f = R.random_frames(N, H, W, seed)
    if N >= 3:
        f[2] = np.where(f[2] < 128, 0, 255).astype(np.uint8)
    return f


def run_f2p(ops, frames, Rr, P, dtype, with_crop=True):
    """One guarded call -> (arena, out view, crop view or None)."""
    from vct_amd import vision as V
    N, H, W, _ = frames.shape
    G_ = Rr // P
    specs = [("out", N * G_ * G_, 3 * P * P, dtype, 3 * P * P, 0)]
    if with_crop:
        specs.append(("crop", N * Rr, Rr * 3, torch.uint8, Rr * 3, 0))
    ar = Arena(specs)
    tables = V.device_tables(H, W, Rr, DEV)
    lut = V.value_table(V.CLIP_MEAN, V.CLIP_STD, dtype).to(DEV)
    crop = ar["crop"].view(N, Rr, Rr, 3) if with_crop else None
    ops.frames_to_patches(torch.from_numpy(frames).to(DEV), tables, lut, P, ar["out"], crop)
    torch.cuda.synchronize()
    ar.check()
    return ar, ar["out"], crop


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("case", F2P_CASES, ids=[f"{c[0]}x{c[1]}-R{c[2]}-P{c[3]}" for c in F2P_CASES])
def test_frames_to_patches(ops, case, dtype):
    H, W, Rr, P = case
    lut = R.value_table(dtype=dtype)
    for N in (1, 3):
        frames = f2p_frames(N, H, W, seed=H + W + N)
        _ar, out, crop = run_f2p(ops, frames, Rr, P, dtype)
        R.check_crop(crop, frames, Rr)                       # PIL is the arbiter
        R.check_patches(out, crop, lut, P)
        _ar2, out2, crop2 = run_f2p(ops, frames, Rr, P, dtype)
        assert torch.equal(out.view(torch.uint8), out2.view(torch.uint8)) and torch.equal(crop, crop2), "a second call gave different bits"
        _ar3, out3, _none = run_f2p(ops, frames, Rr, P, dtype, with_crop=False)       # the optional output left out
        assert torch.equal(out.view(torch.uint8), out3.view(torch.uint8))


@pytest.mark.parametrize("dtype", DT)
def test_frames_to_patches_constant_frames(ops, dtype):
    """All-0 and all-255 frames: the weights of a window do not sum to 2^22 exactly, so 255 * sum can pass 255 * 2^22 -- the clamp."""
    lut = R.value_table(dtype=dtype)
    for H, W in ((100, 37), (20, 31)):
        frames = np.stack([np.zeros((H, W, 3), np.uint8), np.full((H, W, 3), 255, np.uint8)])
        _ar, out, crop = run_f2p(ops, frames, 32, 16, dtype)
        R.check_crop(crop, frames, 32)
        assert bool((crop[0] == 0).all()) and bool((crop[1] == 255).all())
        R.check_patches(out, crop, lut, 16)


def test_frames_to_patches_refusals_launch_nothing(ops):
    """Every refusal is a code and the outputs keep their fill."""
    from vct_amd import _lib, vision as V
    lib = _lib.load()
    H, W, Rr, P = 40, 56, 32, 16
    t = V.device_tables(H, W, Rr, DEV)
    lut = V.value_table(V.CLIP_MEAN, V.CLIP_STD, F32).to(DEV)
    frames = torch.zeros(1, H, W, 3, dtype=torch.uint8, device=DEV)
    ar = Arena([("out", 4, 768, F32, 768, 0), ("crop", 32, 96, torch.uint8, 96, 0)])
    kx, ky, rows = t["hx_w"].shape[1], t["vy_w"].shape[1], t["stage_rows"][P]

    def call(**kw):
        a = dict(dt=0, N=1, H=H, W=W, R=Rr, P=P, frames=frames.data_ptr(), hm=t["hx_min"].data_ptr(), hl=t["hx_len"].data_ptr(),
                 hw=t["hx_w"].data_ptr(), kx=kx, vm=t["vy_min"].data_ptr(), vl=t["vy_len"].data_ptr(), vw=t["vy_w"].data_ptr(), ky=ky,
                 rows=rows, lut=lut.data_ptr(), out=ar["out"].data_ptr(), crop=ar["crop"].data_ptr())
        a.update(kw)
        return lib.vct_frames_to_patches(a["dt"], a["N"], a["H"], a["W"], a["R"], a["P"], a["frames"], a["hm"], a["hl"], a["hw"], a["kx"],
                                         a["vm"], a["vl"], a["vw"], a["ky"], a["rows"], a["lut"], a["out"], a["crop"], _lib.stream_ptr())
    ARG, SHAPE, ALIGN = -1, -2, -3
    for k in ("frames", "hm", "hl", "hw", "vm", "vl", "vw", "lut", "out"):
        assert call(**{k: None}) == ARG, k
    assert call(dt=2) == ARG
    assert call(R=40) == SHAPE                                  # R % P
    assert call(H=0) == SHAPE and call(W=0) == SHAPE and call(N=0) == SHAPE
    assert call(P=8, rows=4000, H=4000) == SHAPE                # the window does not fit the staging
    assert call(P=12, R=24) == ALIGN
    assert call(out=ar["out"].data_ptr() + 4) == ALIGN and call(crop=ar["crop"].data_ptr() + 1) == ALIGN
    assert call(hw=t["hx_w"].data_ptr() + 2) == ALIGN
    torch.cuda.synchronize()
    assert bool((ar.buf[ar.guards[0][1]:ar.guards[1][0]] == 0xFF).all()) and bool((ar["crop"] == 0xFF).all()), "a refused call wrote"
    with pytest.raises(ValueError, match="VCT_E_SHAPE"):
        ops.frames_to_patches(frames, {**t, "stage_rows": {P: 4000}}, lut, P, ar["out"])


# ---- vct_vit_embed / vct_vit_pool ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [4, 64, 768, 1024])
def test_vit_embed(ops, d):
    gam, bet = 1 + 0.2 * rnd(d, seed=d + 1), 0.3 * rnd(d, seed=d + 2)
    for L, N in ((2, 1), (5, 3), (50, 3), (64, 2)):
        e = rnd(N * (L - 1), d, seed=L + d, scale=1.5) + 0.3
        cls, pos = rnd(d, seed=L + d + 1, scale=0.5), rnd(L, d, seed=L + d + 2, scale=0.3)
        outs = []
        for _rep in range(2):
            ar = Arena([("x", N * L, d, F32, d, 0)])
            ops.vit_embed(e, cls, pos, gam, bet, ar["x"])
            torch.cuda.synchronize()
            ar.check()
            outs.append(ar["x"].clone())
        assert torch.equal(outs[0], outs[1]), "a second identical call gave different bits"
        R.check_embed(f"vit_embed d={d} L={L} N={N}", outs[0], e, cls, pos, gam, bet)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("d", [4, 64, 768, 1024])
def test_vit_pool(ops, d, dtype):
    gam, bet = 1 + 0.2 * rnd(d, seed=d + 3), 0.3 * rnd(d, seed=d + 4)
    for L, N in ((2, 1), (5, 3), (50, 9), (64, 2)):
        x = torch.full((N * L, d), NAN, device=DEV)             # NaN in every row the pool must not read
        x[::L] = rnd(N, d, seed=L + d, scale=2.0) - 0.4
        outs = []
        for _rep in range(2):
            ar = Arena([("y", N, d, dtype, d, 0)])
            ops.vit_pool(x, L, gam, bet, ar["y"])
            torch.cuda.synchronize()
            ar.check()
            outs.append(ar["y"].clone())
        assert torch.equal(outs[0], outs[1])
        R.check_pool(f"vit_pool d={d} L={L} N={N} {dtype}", outs[0], x, L, gam, bet)


# ---- the tower ---------------------------------------------------------------------------------------------------------------------------------
TOWERS = {
    # name: (W, heads, ff, layers, P_out, patch, R, std, frames (N, H, W))
    "w64-L5": (64, 2, 128, 2, 48, 16, 32, 0.1, (3, 40, 56)),
    "w128-L50": (128, 2, 256, 1, 40, 16, 112, 0.08, (2, 150, 120)),
}
_CACHE = {}


def case(name):
    """(state dict, frames uint8 [N, H, W, 3], exact fp64 features, heads), computed once per shape."""
    if name not in _CACHE:
        W, H, ff, nl, Po, P, Rr, std, (N, fh, fw) = TOWERS[name]
        sd = R.random_state_dict(W, ff, nl, Po, P, Rr, seed=len(name) + W, std=std)
        frames = torch.from_numpy(R.random_frames(N, fh, fw, seed=W + 1))
        _CACHE[name] = (sd, frames, R.tower(sd, frames, H), H)
    return _CACHE[name]


def gemm_bound(ref, x, w, bias, dtype_out, addend=None, act=False):
    """tests/gemm_ref.py's bound for ref = epilogue(x @ w^T + bias) [+ addend], from fp64 copies of the operands as stored."""
    K = x.shape[1]
    acc = (K + 1) * G.U24 * (x.abs() @ w.abs().t() + bias.abs())
    b = U[dtype_out] * ref.abs() + (1.1 if act else 1.0) * acc
    if act:
        z = x @ w.t() + bias
        b = b + G.U20 * TR.quick_gelu(z).abs() * (1 + z.abs())
    if addend is not None:
        b = b + U[dtype_out] * addend.abs()
    return b


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("name", list(TOWERS))
def test_tower_stage_by_stage(ops, name, dtype):
    from vct_amd.vision import ClipVisionTower
    sd, frames, _exact, H = case(name)
    t = ClipVisionTower.from_state_dict(sd, DEV, dtype, heads=H)
    out = t.encode_frames(frames, keep=True)
    k = t.kept
    torch.cuda.synchronize()
    N, L, P, Rr = frames.shape[0], t.rows, t.patch, t.resolution
    assert L == (Rr // P) ** 2 + 1 == TOWERS[name][6] ** 2 // P ** 2 + 1
    R.check_crop(k["crop"], frames, Rr)
    R.check_patches(k["a"], k["crop"], R.value_table(dtype=dtype), P)
    zero = lambda n: torch.zeros(n, dtype=F64, device=DEV)      # noqa: E731
    a, conv = d64(k["a"]), d64(t.conv)
    ref = a @ conv.t()
    R.check_elem(f"{name} {dtype} patch embedding", k["e"], ref, gemm_bound(ref, a, conv, zero(conv.shape[0]), F32))
    R.check_embed(f"{name} {dtype} class / position / ln_pre", k["x0"], k["e"], t.cls, t.pos, t.lnpre_g, t.lnpre_b)
    x = d64(k["x0"])
    for li, (kl, lw) in enumerate(zip(k["layers"], t.lw)):
        w = {n: d64(v) for n, v in lw.items()}
        tag = f"{name} {dtype} layer {li}"
        ref = TR.layer_norm(x, w["ln1_g"], w["ln1_b"])
        R.check_elem(f"{tag} ln_1", kl["h1"], ref, R.ln_bound(ref, dtype))
        h1 = d64(kl["h1"])
        ref = h1 @ w["w_qkv"].t() + w["b_qkv"]
        R.check_elem(f"{tag} qkv", kl["qkv"], ref, gemm_bound(ref, h1, w["w_qkv"], w["b_qkv"], dtype))
        ref = R.attention(d64(kl["qkv"]), N, L, H)
        e = relf(kl["o"], ref)
        print(f"[vision-tower] {tag} attention (no mask, L = {L}): rel-Frobenius {e:.3e}")
        assert e <= (1.5e-2 if dtype == BF else 2e-5)
        o = d64(kl["o"])
        ref = x + o @ w["w_o"].t() + w["b_o"]
        R.check_elem(f"{tag} out_proj + stream", kl["x1"], ref, gemm_bound(ref, o, w["w_o"], w["b_o"], F32, addend=x))
        x1 = d64(kl["x1"])
        ref = TR.layer_norm(x1, w["ln2_g"], w["ln2_b"])
        R.check_elem(f"{tag} ln_2", kl["h2"], ref, R.ln_bound(ref, dtype))
        h2 = d64(kl["h2"])
        ref = TR.quick_gelu(h2 @ w["w_fc"].t() + w["b_fc"])
        R.check_elem(f"{tag} c_fc + QuickGELU", kl["f"], ref, gemm_bound(ref, h2, w["w_fc"], w["b_fc"], dtype, act=True))
        f = d64(kl["f"])
        ref = x1 + f @ w["w_proj"].t() + w["b_proj"]
        R.check_elem(f"{tag} c_proj + stream", kl["x2"], ref, gemm_bound(ref, f, w["w_proj"], w["b_proj"], F32, addend=x1))
        x = d64(kl["x2"])
    R.check_pool(f"{name} {dtype} ln_post of the class rows", k["pooled"], k["layers"][-1]["x2"], L, t.lnpost_g, t.lnpost_b)
    pooled, proj = d64(k["pooled"]), d64(t.proj)
    ref = pooled @ proj.t()
    R.check_elem(f"{name} {dtype} projection", out, ref, gemm_bound(ref, pooled, proj, zero(proj.shape[0]), F32))
    assert torch.equal(out, k["out"]) and out.dtype == F32 and tuple(out.shape) == (N, t.dim)
    assert torch.equal(t.encode_frames(frames), out), "a second identical call gave different bits"
    assert torch.equal(t.encode_frames(frames.to(DEV)), out), "device-resident frames gave different bits"
    allc = Arena([("all", N, t.dim, F32, t.dim, 0)])
    t.encode_all(frames, chunk=2, out=allc["all"])
    torch.cuda.synchronize()
    allc.check()
    if N > 2:       # the last chunk holds one frame: the GEMMs may take another route for it, so to the end-to-end bound's scale only
        assert relf(allc["all"], d64(out)) <= (1e-3 if dtype == F32 else 3e-2)
    else:
        assert torch.equal(allc["all"], out)


def torch_module_error(sd_hf, shape, heads, frames, dtype, exact):
    """Relative error of transformers' own CPU module, run in `dtype` on CLIP's preprocessing of the frames, against the same fp64
    result -- printed beside the tower's; None where transformers is not installed."""
    try:
        from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
    except ImportError:
        return None
    W, ff, nl, Po, P, Rr = shape
    cfg = CLIPVisionConfig(hidden_size=W, intermediate_size=ff, num_hidden_layers=nl, num_attention_heads=heads, image_size=Rr,
                           patch_size=P, projection_dim=Po, hidden_act="quick_gelu")
    m = CLIPVisionModelWithProjection(cfg).eval()
    m.load_state_dict({k: torch.as_tensor(v).float() for k, v in sd_hf.items()}, strict=False)
    m = m.to(dtype)
    crop = np.stack([R.preprocess_u8(f, Rr) for f in np.asarray(frames)])
    lut = R.value_table(dtype=dtype)
    pixels = torch.stack([lut[c][torch.from_numpy(crop[..., c]).long()] for c in range(3)], 1)
    with torch.no_grad():
        got = m(pixel_values=pixels).image_embeds
    return relf(got, exact.cpu())


@pytest.mark.parametrize("dtype", DT)
def test_end_to_end_against_the_exact_restatement(ops, dtype):
    from vct_amd.vision import ClipVisionTower
    bound = 1e-3 if dtype == F32 else 3e-2
    tol = GradTol("vision_tower_end_to_end", dtype, bound)
    theirs = {}
    for name in TOWERS:
        sd, frames, exact, H = case(name)
        W, _h, ff, nl, Po, P, Rr = TOWERS[name][:7]
        theirs[name] = torch_module_error(R.openai_to_transformers(sd), (W, ff, nl, Po, P, Rr), H, frames, dtype, exact)
        t = ClipVisionTower.from_state_dict(sd, DEV, dtype, heads=H)
        err = relf(t.encode_frames(frames), exact.to(DEV))
        print(f"[vision-tower] end to end {name} {dtype}: tower {err:.3e}, torch's CPU module in the same dtype {theirs[name]}, bound {bound}")
        tol.add(name, err)
    # the recorded transformers model (3 layers; tests/golden/vision_tower.npz), from transformers' key convention
    z = load_golden("vision_tower.npz")
    sd = {k[2:]: torch.from_numpy(z[k]).to(F64) * float(z["scale/" + k[2:]]) for k in z.files if k.startswith("q/")}
    exact = torch.from_numpy(z["out"])
    t = ClipVisionTower.from_state_dict(sd, DEV, dtype, heads=int(z["heads"]))
    got = t.encode_frames(torch.from_numpy(z["frames"]), keep=True)
    assert torch.equal(t.kept["crop"].cpu(), torch.from_numpy(z["crop"])), "the cropped image is not the recorded PIL one"
    err = relf(got, exact.to(DEV))
    theirs["golden"] = torch_module_error(sd, (64, 128, 3, 48, 16, 32), int(z["heads"]), z["frames"], dtype, exact)
    print(f"[vision-tower] end to end golden-transformers {dtype}: tower {err:.3e}, torch's CPU module in the same dtype {theirs['golden']}, "
          f"bound {bound}")
    tol.add("golden-transformers", err)
    print("[vision-tower] end to end:", tol.errs, "torch CPU module:", theirs)
    tol.report()


def test_tower_is_recorded_by_a_launch_list(ops):
    """Every launch of the forward goes through the runtime's wrapper: a launch list records 7 per layer + 5 and replays them."""
    from vct_amd.vision import ClipVisionTower
    sd, frames, _exact, H = case("w64-L5")
    t = ClipVisionTower.from_state_dict(sd, DEV, BF, heads=H)
    fdev = frames.to(DEV)
    want = t.encode_frames(fdev).clone()
    out = torch.zeros_like(want)
    ll = ops.LaunchList()
    with ll.record():
        t.encode_frames(fdev, out=out)
    assert len(ll) == 7 * t.layers + 5, len(ll)
    out.zero_()
    ll.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    ll.close()


# ---- frames to captions --------------------------------------------------------------------------------------------------------------------------
def caption_model(dim, dtype=F32, extra_modal=None):
    """The tiny caption model of the multi-modal tests with modal_shape = [dim] (+ a second stream)."""
    from helpers import build_model
    from mm_ref import mm_config, mm_params
    mc = mm_config(128, [dim] + ([extra_modal] if extra_modal else []), 4, 256, 1, 2)
    mc["matching"] = None
    return build_model(mc, 211, DEV, dtype, mm_params(mc, 211, 3))


def spy_ids(model, name, log):
    """Wrap model.<name> so that every id matrix it returns is appended to `log`."""
    inner = getattr(model, name)

    def wrapped(*a, **kw):
        ids = inner(*a, **kw)
        log.append((ids[0] if isinstance(ids, tuple) else ids).clone())      # (ids, maps) with return_attn
        return ids
    setattr(model, name, wrapped)


@pytest.mark.parametrize("beam", [None, 2], ids=["greedy", "beam2"])
def test_v2t_frames_equals_v2t_batch_on_separately_encoded_features(ops, beam):
    """Two videos of 3 and 5 frames, 40 x 56 and 64 x 48: the ids are bitwise those of v2t_batch on features from separate
    encode_frames calls, padded here with torch."""
    from vct_amd import evaluate
    from vct_amd.vision import ClipVisionTower
    sd, _frames, _exact, H = case("w64-L5")
    tower = ClipVisionTower.from_state_dict(sd, DEV, F32, heads=H)
    model = caption_model(tower.dim)
    videos = [torch.from_numpy(R.random_frames(3, 40, 56, seed=5)), torch.from_numpy(R.random_frames(5, 64, 48, seed=6)).to(DEV)]
    log = []
    spy_ids(model, "greedy_decode_ids" if beam is None else "beam_decode_ids", log)
    got = evaluate.v2t_frames(model, tower, videos, max_len=8, beam_size=beam)
    feats = torch.zeros(2, 5, tower.dim, device=DEV)
    feats[0, :3], feats[1] = tower.encode_frames(videos[0]), tower.encode_frames(videos[1])
    mask = torch.tensor([[False, False, False, True, True], [False] * 5], device=DEV)
    want = evaluate.v2t_batch(model, [feats], [mask], max_len=8, beam_size=beam)
    assert len(log) == 2 and torch.equal(log[0], log[1]), "the id matrices differ"
    assert got == want and len(got) == 2 and all(isinstance(c, str) for c in got)
    with pytest.raises(ValueError, match="modal_shape"):
        evaluate.v2t_frames(caption_model(tower.dim + 16), tower, videos, max_len=8)
    if beam is None:
        caps, maps = evaluate.v2t_frames(model, tower, videos, max_len=8, return_attn=True)
        assert caps == got and maps.shape[0] == 2
        # a second feature stream is passed through
        m2 = caption_model(tower.dim, extra_modal=32)
        other = rnd(2, 4, 32, seed=8)
        a = evaluate.v2t_frames(m2, tower, videos, max_len=8, extra_feats=[other])
        b = evaluate.v2t_batch(m2, [feats, other], [mask, torch.zeros(2, 4, dtype=torch.bool, device=DEV)], max_len=8)
        assert a == b
        with pytest.raises(ValueError, match="extra_feats"):
            evaluate.v2t_frames(m2, tower, videos, max_len=8)
