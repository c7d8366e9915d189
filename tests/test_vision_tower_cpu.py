"""The CLIP vision tower without a GPU: the integer resize restatement (tests/vision_ref.py) against PIL, the package's coefficient and
value tables against the restatement and against torch's arithmetic, the fp64 tower against transformers' module and the recorded fixture
(tests/golden/vision_tower.npz, tools/make_golden_vision_tower.py), the two key conventions, every refusal of the loader, the Python
surface and the new entry points, and the GPU file's checkers against seeded faults."""
import ctypes

import numpy as np
import pytest
import torch

import text_tower_ref as TR
import vision_ref as R
from helpers import load_golden

F64 = torch.float64


def golden():
    z = load_golden("vision_tower.npz")
    sd = {k[2:]: torch.from_numpy(z[k]).to(F64) * float(z["scale/" + k[2:]]) for k in z.files if k.startswith("q/")}
    return sd, z["frames"], z["crop"], torch.from_numpy(z["out"]), int(z["heads"])


def maxrel(a, b):
    return float((a - b).abs().max() / b.abs().max())


# ---- the resize -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", R.SIZES, ids=[f"{h}x{w}-R{r}" for h, w, r in R.SIZES])
def test_resize_restatement_equals_pil(size):
    """PIL is the arbiter: the whole resized image (not only the crop) in every byte, and the crop through PIL's own crop."""
    Image = pytest.importorskip("PIL.Image")
    H, W, Rr = size
    img = R.random_frames(1, H, W, seed=H * W)[0]
    oh, ow = R.resized_size(H, W, Rr)
    assert min(oh, ow) == Rr and (oh == Rr) == (H <= W)
    ref = np.asarray(Image.fromarray(img).resize((ow, oh), Image.BICUBIC))
    assert np.array_equal(R.resize(img, oh, ow), ref)
    assert np.array_equal(R.preprocess_u8(img, Rr), R.pil_preprocess_u8(img, Rr))
    sharp = np.where(img < 128, 0, 255).astype(np.uint8)                     # overshoot on both sides: the clamp
    assert np.array_equal(R.resize(sharp, oh, ow), np.asarray(Image.fromarray(sharp).resize((ow, oh), Image.BICUBIC)))


def test_size_and_crop_rules():
    from vct_amd import vision as V
    for H, W, Rr in R.SIZES + [(32, 45, 32), (32, 50, 32), (1080, 1920, 224)]:
        assert V.resized_size(H, W, Rr) == R.resized_size(H, W, Rr)
        assert V.crop_offsets(*R.resized_size(H, W, Rr), Rr) == R.crop_offsets(*R.resized_size(H, W, Rr), Rr)
    assert R.resized_size(360, 640, 224) == (224, 398) and R.crop_offsets(224, 398, 224) == (0, 87)
    assert R.resized_size(20, 31, 32) == (32, 49) and R.crop_offsets(32, 49, 32) == (0, 8)        # 8.5 -> 8: half to even
    assert R.crop_offsets(32, 45, 32) == (0, 6) and R.crop_offsets(32, 47, 32) == (0, 8)           # 6.5 -> 6, 7.5 -> 8
    assert R.resized_size(100, 37, 32) == (86, 32) and R.crop_offsets(86, 32, 32) == (27, 0)


@pytest.mark.parametrize("size", R.SIZES + [(32, 45, 32), (1080, 1920, 224)], ids=lambda s: f"{s[0]}x{s[1]}-R{s[2]}")
def test_coefficient_tables(size):
    """vision.py's tables are the restatement's, applying them (as the kernel does: horizontal taps, uint8, vertical taps) gives the
    restatement's image, and no accumulator can leave int32: 2^21 + 255 * sum |w| < 2^31 for every window."""
    from vct_amd import vision as V
    H, W, Rr = size
    mine, ref = V.resize_tables(H, W, Rr), R.tables(H, W, Rr)
    for k, v in ref.items():
        assert mine[k].dtype == np.int32 and np.array_equal(mine[k], v), k
    for p in ("hx", "vy"):
        w, n, lo = mine[p + "_w"].astype(np.int64), mine[p + "_len"], mine[p + "_min"]
        assert int((1 << 21) + 255 * np.abs(w).sum(1).max()) < 2 ** 31
        assert all((w[i, n[i]:] == 0).all() for i in range(Rr)) and (n >= 1).all() and (lo >= 0).all()
        assert (lo + n <= (W if p == "hx" else H)).all() and (np.diff(lo) >= 0).all()
    if H * W <= 640 * 360:
        img = R.random_frames(1, H, W, seed=7)[0].astype(np.int64)
        taps = lambda src, p: np.stack([np.clip((((src[:, mine[p + "_min"][i]:mine[p + "_min"][i] + mine[p + "_len"][i]]      # noqa: E731
                                                   * mine[p + "_w"][i, :mine[p + "_len"][i], None].astype(np.int64)).sum(1)
                                                  + (1 << 21)) >> 22), 0, 255) for i in range(Rr)], 1)
        got = taps(taps(img, "hx").transpose(1, 0, 2), "vy").transpose(1, 0, 2)
        assert np.array_equal(got.astype(np.uint8), R.preprocess_u8(img.astype(np.uint8), Rr))
    P = 32 if Rr == 224 else 16
    rows = V.stage_rows(mine, P)
    assert rows == max(int(ref["vy_min"][g + P - 1] + ref["vy_len"][g + P - 1] - ref["vy_min"][g]) for g in range(0, Rr, P)) <= H
    assert V.staging_bytes(mine, P) <= V.LDS_BYTES


def test_value_table_is_torchs_arithmetic():
    """Bit for bit ToTensor / Normalize as torchvision computes them (restated in vision_ref.value_table from its source: this image has
    no torchvision), torch's cast for bf16, and other means / stds."""
    from vct_amd import vision as V
    for mean, std in ((V.CLIP_MEAN, V.CLIP_STD), ((0.5, 0.5, 0.5), (0.5, 0.25, 0.125)), ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))):
        a, b = V.value_table(mean, std), R.value_table(mean, std)
        assert a.dtype == torch.float32 and tuple(a.shape) == (3, 256) and torch.equal(a.view(torch.int32), b.view(torch.int32))
        # ... and element by element, the way a per-pixel pipeline would
        for c in range(3):
            for v in (0, 1, 127, 128, 254, 255):
                want = (torch.tensor(v, dtype=torch.uint8).to(torch.float32).div(255) - torch.tensor(mean[c], dtype=torch.float32)) \
                    / torch.tensor(std[c], dtype=torch.float32)
                assert a[c, v].item() == want.item()
        h = V.value_table(mean, std, torch.bfloat16)
        assert h.dtype == torch.bfloat16 and torch.equal(h.view(torch.int16), a.to(torch.bfloat16).view(torch.int16))
    assert V.CLIP_MEAN == R.CLIP_MEAN and V.CLIP_STD == R.CLIP_STD


# ---- the tower reference ----------------------------------------------------------------------------------------------------------------
def hf_module(sd_hf, W, ff, nl, heads, Po, P, Rr):
    tr = pytest.importorskip("transformers")
    cfg = tr.CLIPVisionConfig(hidden_size=W, intermediate_size=ff, num_hidden_layers=nl, num_attention_heads=heads, image_size=Rr,
                              patch_size=P, projection_dim=Po, hidden_act="quick_gelu")
    m = tr.CLIPVisionModelWithProjection(cfg).double().eval()
    res = m.load_state_dict({k: torch.as_tensor(v).double() for k, v in sd_hf.items()}, strict=False)
    assert not res.unexpected_keys and all("position_ids" in k for k in res.missing_keys), res
    return m


def pixel_values(frames, Rr):
    crop = np.stack([R.pil_preprocess_u8(f, Rr) for f in frames])
    lut = R.value_table()
    return torch.stack([lut[c][torch.from_numpy(crop[..., c]).long()] for c in range(3)], 1).double()


def test_restatement_reproduces_the_fixture():
    """The recorded outputs are transformers' own (fp64) on PIL's preprocessing; the restatement must agree to 1e-12 -- the criterion of
    tests/test_text_tower_cpu.py -- and its cropped image must be the recorded PIL one."""
    sd, frames, crop, out, H = golden()
    got, kept = R.tower(sd, frames, H, keep=True)
    assert np.array_equal(kept["crop"].numpy(), crop)
    assert maxrel(got, out) <= 1e-12


def test_restatement_against_transformers_golden():
    sd, frames, _crop, out, H = golden()
    m = hf_module(sd, 64, 128, 3, H, 48, 16, 32)
    with torch.no_grad():
        ref = m(pixel_values=pixel_values(frames, 32)).image_embeds
    assert maxrel(ref, out) <= 1e-12                       # the fixture is what the module computes today
    assert maxrel(R.tower(sd, frames, H), ref) <= 1e-12


@pytest.mark.parametrize("convention,prefix", [("openai", ""), ("transformers", ""), ("openai", "clip."), ("transformers", "clip.")])
def test_restatement_against_transformers_random(convention, prefix):
    """Random weights, both key conventions, with and without a prefix; L = 50 rows (the real count) and two heads."""
    oa = R.random_state_dict(64, 128, 2, 40, 16, 112, seed=11)
    sd = R.random_state_dict(64, 128, 2, 40, 16, 112, seed=11, convention=convention, prefix=prefix)
    frames = R.random_frames(2, 150, 120, seed=12)
    m = hf_module(R.openai_to_transformers(oa), 64, 128, 2, 2, 40, 16, 112)
    with torch.no_grad():
        ref = m(pixel_values=pixel_values(frames, 112)).image_embeds
    assert maxrel(R.tower(sd, frames, 2, prefix=prefix), ref) <= 1e-12


def test_key_conventions_through_the_package():
    """The package's canonical form is the same from both conventions and under a prefix, and is what the restatement reads."""
    from vct_amd import vision as V
    oa = R.random_state_dict(64, 128, 2, 48, 16, 32, seed=3)
    hf = R.openai_to_transformers(oa)
    a, b = V.canonical_vision_weights(oa), V.canonical_vision_weights(hf)
    c = V.canonical_vision_weights({"clip." + k: v for k, v in hf.items()}, prefix="clip.")
    w = R.weights(oa)
    for k in ("conv", "cls", "pos", "lnpre_g", "lnpre_b", "lnpost_g", "lnpost_b", "proj"):
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), k
        assert torch.equal(a[k].double(), w[k] if k != "proj" else w[k].t()), k
    assert a["patch"] == b["patch"] == 16 and tuple(a["conv"].shape) == (64, 768) and tuple(a["proj"].shape) == (48, 64)
    for la, lb, lr in zip(a["layers"], b["layers"], w["layers"]):
        assert all(torch.equal(la[k], lb[k]) and torch.equal(la[k].double(), lr[k]) for k in la)
    # fp16 weights (what clip.load leaves on a GPU) convert exactly
    half = {k: v.half() for k, v in oa.items()}
    assert torch.equal(V.canonical_vision_weights(half)["cls"], oa["visual.class_embedding"].half().float())
    frames = R.random_frames(2, 40, 56, seed=4)
    assert maxrel(R.tower(hf, frames, 2), R.tower(oa, frames, 2)) <= 1e-12


def test_emulation_rounds_and_stays_close():
    sd = R.random_state_dict(64, 128, 2, 48, 16, 32, seed=5)
    frames = R.random_frames(3, 40, 56, seed=6)
    a, b = R.tower(sd, frames, 2), R.tower(sd, frames, 2, emulate=True)
    err = float((a - b).norm() / a.norm())
    assert 1e-4 < err < 3e-2, err


# ---- the loader and the Python surface --------------------------------------------------------------------------------------------------
def test_loader_reads_shapes_and_refuses_bad_dicts(tmp_path):
    from vct_amd.vision import ClipVisionTower
    oa = R.random_state_dict(64, 128, 2, 48, 16, 32, seed=3)
    t = ClipVisionTower.from_state_dict(oa, "cpu", torch.float32, heads=2)
    assert (t.width, t.heads, t.layers, t.ff, t.dim, t.patch, t.resolution, t.rows, t.grid) == (64, 2, 2, 128, 48, 16, 32, 5, 2)
    assert ClipVisionTower.from_state_dict(oa, "cpu", torch.float32).heads == 1          # CLIP's own rule: W // 64
    t16 = ClipVisionTower.from_state_dict(R.openai_to_transformers(oa), "cpu", heads=2)
    assert t16.conv.dtype == t16.lw[0]["w_qkv"].dtype == t16.proj.dtype == t16.lut.dtype == torch.bfloat16
    assert t16.cls.dtype == t16.pos.dtype == t16.lnpre_g.dtype == t16.lw[0]["b_qkv"].dtype == torch.float32
    assert torch.equal(t16.conv, oa["visual.conv1.weight"].reshape(64, -1).to(torch.bfloat16))
    assert torch.equal(t16.proj.float(), oa["visual.proj"].t().to(torch.bfloat16).float())
    path = tmp_path / "clip.pt"
    torch.save({"clip." + k: v for k, v in oa.items()}, path)
    assert ClipVisionTower.from_file(str(path), "cpu", torch.float32, heads=2, prefix="clip.").dim == 48
    for conv in ("openai", "transformers"):
        sd = oa if conv == "openai" else R.openai_to_transformers(oa)
        for key in list(sd):
            if not key.startswith("vis"):
                continue
            with pytest.raises(ValueError, match=key.replace(".", r"\.")):
                ClipVisionTower.from_state_dict({k: v for k, v in sd.items() if k != key}, "cpu", heads=2)
        key = [k for k in sd if k.endswith("out_proj.weight")][0]
        with pytest.raises(ValueError, match="out_proj"):
            ClipVisionTower.from_state_dict({**sd, key: sd[key][:, :60]}, "cpu", heads=2)
        key = [k for k in sd if "position" in k][0]
        with pytest.raises(ValueError, match="position"):
            ClipVisionTower.from_state_dict({**sd, key: sd[key][:4]}, "cpu", heads=2)                 # 4 rows: no G * G + 1
    with pytest.raises(ValueError, match="conv1"):
        ClipVisionTower.from_state_dict({"x": torch.zeros(1)}, "cpu")
    with pytest.raises(ValueError, match="prefix 'clip.'"):
        ClipVisionTower.from_state_dict(oa, "cpu", prefix="clip.")
    with pytest.raises(ValueError, match="heads"):
        ClipVisionTower.from_state_dict(oa, "cpu", heads=3)
    with pytest.raises(ValueError, match="compute_dtype"):
        ClipVisionTower.from_state_dict(oa, "cpu", torch.float16, heads=2)


def test_towers_the_kernels_cannot_take_are_refused_at_construction():
    """ViT-B/16 (197 rows) and ViT-L/14 (257): the message names the attention limit; head sizes and widths beyond the kernels'."""
    from vct_amd.vision import ClipVisionTower
    mk = lambda W, patch, Rr, ff=128: R.random_state_dict(W, ff, 1, 32, patch, Rr, seed=1)      # noqa: E731
    with pytest.raises(ValueError, match=r"197 rows.*at most 64.*attention"):
        ClipVisionTower.from_state_dict(mk(64, 16, 224), "cpu")
    with pytest.raises(ValueError, match=r"257 rows.*at most 64.*attention"):
        ClipVisionTower.from_state_dict(mk(64, 14, 224), "cpu")
    ClipVisionTower.from_state_dict(mk(64, 32, 224), "cpu")                                      # ViT-B/32's 50 rows fit
    with pytest.raises(ValueError, match="head size 12"):
        ClipVisionTower.from_state_dict(mk(48, 16, 32), "cpu", heads=4)
    with pytest.raises(ValueError, match="head size 256"):
        ClipVisionTower.from_state_dict(mk(256, 16, 32), "cpu", heads=1)
    with pytest.raises(ValueError, match="width 1088"):
        ClipVisionTower.from_state_dict(mk(1088, 16, 32), "cpu")
    with pytest.raises(ValueError, match="patch size 12"):
        ClipVisionTower.from_state_dict(mk(64, 12, 24), "cpu")


def test_python_refusals_before_any_device_work():
    from vct_amd import evaluate
    from vct_amd.vision import ClipVisionTower
    t = ClipVisionTower.from_state_dict(R.random_state_dict(64, 128, 1, 48, 16, 32, seed=3), "cpu", torch.float32, heads=2)
    ok = torch.zeros(2, 40, 56, 3, dtype=torch.uint8)
    for bad in (ok.float(), ok[0], ok[..., :2], torch.zeros(0, 4, 4, 3, dtype=torch.uint8), [[1, 2]]):
        with pytest.raises(ValueError, match="frames must be"):
            t.encode_frames(bad)
    with pytest.raises(ValueError, match="out must be"):
        t.encode_frames(ok, out=torch.zeros(2, 47))
    with pytest.raises(ValueError, match="chunk"):
        t.encode_all(ok, chunk=0)
    with pytest.raises(ValueError, match="staging"):                  # 16 output rows of a 20 000-row frame: 10 000 staged rows, far over 64 KB
        t.encode_frames(torch.empty(1, 20000, 20000, 3, dtype=torch.uint8, device="meta"))

    class Model:
        model_config = {"modal_shape": [64]}
    with pytest.raises(ValueError, match="48.*64|64.*48"):
        evaluate.v2t_frames(Model(), t, [ok])
    Model.model_config = {"modal_shape": [48, 16]}
    with pytest.raises(ValueError, match="extra_feats"):
        evaluate.v2t_frames(Model(), t, [ok])
    Model.model_config = {"modal_shape": [48]}
    with pytest.raises(ValueError, match="videos"):
        evaluate.v2t_frames(Model(), t, [])


# ---- the C entry points -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from vct_amd import _lib
    return _lib.load()


def test_abi_is_additive(lib):
    from vct_amd import _lib
    assert {"vct_frames_to_patches", "vct_vit_embed", "vct_vit_pool"} <= set(_lib.exported_symbols())
    assert lib.vct_abi_version() == _lib.ABI_VERSION == 16
    from vct_amd import ops
    assert all(callable(getattr(ops, n)) for n in ("frames_to_patches", "vit_embed", "vit_pool"))


def test_entry_points_validate_arguments(lib):
    """Codes, before any device use (there is no device here): the pointers are never dereferenced."""
    p = ctypes.c_void_p
    a16, a8, a4, a2, a1 = p(4096), p(4096 + 8), p(4096 + 4), p(4096 + 2), p(4096 + 1)
    ARG, SHAPE, ALIGN = -1, -2, -3

    def f2p(dt=1, N=2, H=40, W=56, Rr=32, P=16, kx=5, ky=5, rows=30, ptrs=None, **kw):
        q = dict(frames=a16, hm=a16, hl=a16, hw=a16, vm=a16, vl=a16, vw=a16, lut=a16, out=a16, crop=a16)
        q.update(kw)
        return lib.vct_frames_to_patches(dt, N, H, W, Rr, P, q["frames"], q["hm"], q["hl"], q["hw"], kx, q["vm"], q["vl"], q["vw"], ky, rows,
                                         q["lut"], q["out"], q["crop"], None)
    for k in ("frames", "hm", "hl", "hw", "vm", "vl", "vw", "lut", "out"):
        assert f2p(**{k: None}) == ARG, k
    assert f2p(dt=2) == ARG
    assert f2p(Rr=40) == SHAPE                                               # R % P
    assert f2p(H=0) == SHAPE and f2p(W=0) == SHAPE and f2p(N=0) == SHAPE and f2p(Rr=0) == SHAPE and f2p(P=0) == SHAPE
    assert f2p(kx=0) == SHAPE and f2p(ky=0) == SHAPE and f2p(rows=0) == SHAPE
    assert f2p(kx=57) == SHAPE and f2p(ky=41) == SHAPE and f2p(rows=41) == SHAPE      # windows larger than the frame
    assert f2p(H=4000, rows=1400) == SHAPE                                   # 16 * 3 * 1400 bytes of staging alone: over 64 KB
    assert f2p(N=2 ** 30, Rr=64) == SHAPE                                    # N * G * G beyond int32
    assert f2p(H=40000, W=40000, rows=30) == SHAPE                           # 3 * H * W beyond int32
    assert f2p(P=12, Rr=24) == ALIGN
    assert f2p(out=a8) == ALIGN and f2p(crop=a2) == ALIGN and f2p(hw=a2) == ALIGN and f2p(vm=a2) == ALIGN
    assert f2p(dt=1, lut=a1) == ALIGN and f2p(dt=0, lut=a2) == ALIGN
    ok = [a16] * 6                                                           # e, cls, pos, gamma, beta, x
    emb = lambda N, L, d, *ptrs: lib.vct_vit_embed(N, L, d, *ptrs, None)      # noqa: E731
    for i in range(6):
        assert emb(2, 5, 64, *[None if j == i else q for j, q in enumerate(ok)]) == ARG
        assert emb(2, 5, 64, *[a8 if j == i else q for j, q in enumerate(ok)]) == ALIGN
    assert emb(2, 5, 1028, *ok) == SHAPE and emb(2, 5, 66, *ok) == ALIGN and emb(2, 5, 0, *ok) == SHAPE
    assert emb(0, 5, 64, *ok) == SHAPE and emb(2, 1, 64, *ok) == SHAPE and emb(2 ** 30, 5, 64, *ok) == SHAPE
    pool = lambda dt, N, L, d, *ptrs: lib.vct_vit_pool(dt, N, L, d, *ptrs, None)      # noqa: E731
    ok = [a16] * 4                                                           # x, gamma, beta, y
    for i in range(4):
        assert pool(1, 2, 5, 64, *[None if j == i else q for j, q in enumerate(ok)]) == ARG
    assert pool(2, 2, 5, 64, *ok) == ARG
    assert pool(1, 2, 5, 1028, *ok) == SHAPE and pool(1, 2, 5, 66, *ok) == ALIGN
    assert pool(1, 0, 5, 64, *ok) == SHAPE and pool(1, 2, 0, 64, *ok) == SHAPE
    assert pool(0, 2, 5, 64, a16, a16, a16, a8) == ALIGN and pool(1, 2, 5, 64, a16, a16, a16, a4) == ALIGN
    assert pool(1, 2, 5, 64, a8, a16, a16, a16) == ALIGN


def test_python_wrappers_check_shapes():
    from vct_amd import ops
    x = torch.zeros(10, 64)
    with pytest.raises(AssertionError):
        ops.vit_pool(x.double(), 5, torch.ones(64), torch.zeros(64), torch.zeros(2, 64))
    with pytest.raises(AssertionError):
        ops.vit_embed(torch.zeros(9, 64), torch.zeros(64), torch.zeros(5, 64), torch.ones(64), torch.zeros(64), x)      # 9 % 4
    with pytest.raises(AssertionError):
        ops.frames_to_patches(torch.zeros(1, 8, 8, 3), {"R": 32}, torch.zeros(3, 256), 16, torch.zeros(4, 768))           # float frames


# ---- the GPU file's checkers reject seeded faults -----------------------------------------------------------------------------------------
def _good():
    frames = R.random_frames(2, 40, 56, seed=9)
    crop = np.stack([R.preprocess_u8(f, 32) for f in frames])
    lut = R.value_table()
    return frames, crop, lut, R.patch_matrix(crop, lut, 16)


def test_checkers_accept_the_right_answer():
    frames, crop, lut, a = _good()
    R.check_crop(crop, frames, 32)
    R.check_patches(a, crop, lut, 16)
    R.check_patches(R.patch_matrix(crop, lut.to(torch.bfloat16), 16), crop, lut.to(torch.bfloat16), 16)


def test_checkers_reject_a_dropped_tap():
    frames, _crop, _lut, _a = _good()

    def dropped(img, Rr):
        oh, ow = R.resized_size(*img.shape[:2], Rr)
        cs = [(x0, k[:-1]) if i == 16 else (x0, k) for i, (x0, k) in enumerate(R.coeffs(img.shape[1], ow))]       # column 16 loses a tap
        t = R.pass1d(R.pass1d(img, ow, cs).transpose(1, 0, 2), oh).transpose(1, 0, 2) if oh != img.shape[0] else R.pass1d(img, ow, cs)
        top, left = R.crop_offsets(oh, ow, Rr)
        return np.ascontiguousarray(t[top:top + Rr, left:left + Rr])
    assert not np.array_equal(dropped(frames[0], 32), R.preprocess_u8(frames[0], 32))
    with pytest.raises(AssertionError, match="differ from PIL"):
        R.check_crop(np.stack([dropped(f, 32) for f in frames]), frames, 32)


def test_checkers_reject_bgr_and_a_shifted_crop():
    frames, crop, lut, _a = _good()
    with pytest.raises(AssertionError, match="differ from PIL"):
        R.check_crop(np.ascontiguousarray(crop[..., ::-1]), frames, 32)
    with pytest.raises(AssertionError, match="lut"):
        R.check_patches(R.patch_matrix(np.ascontiguousarray(crop[..., ::-1]), lut, 16), crop, lut, 16)
    oh, ow = R.resized_size(40, 56, 32)
    top, left = R.crop_offsets(oh, ow, 32)
    shifted = np.stack([np.ascontiguousarray(R.resize(f, oh, ow)[top:top + 32, left + 1:left + 33]) for f in frames])
    with pytest.raises(AssertionError, match="differ from PIL"):
        R.check_crop(shifted, frames, 32)


def test_checkers_reject_the_channel_last_patch_layout():
    _frames, crop, lut, a = _good()
    img = torch.stack([lut[c][torch.from_numpy(crop[..., c]).long()] for c in range(3)], 1)        # [N, 3, R, R]
    wrong = img.view(2, 3, 2, 16, 2, 16).permute(0, 2, 4, 3, 5, 1).reshape(8, 768).contiguous()       # [py][px][c]
    assert wrong.shape == a.shape and not torch.equal(wrong, a)
    with pytest.raises(AssertionError, match="lut"):
        R.check_patches(wrong, crop, lut, 16)


def test_checkers_reject_embed_and_pool_faults():
    g = torch.Generator().manual_seed(1)
    n = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
    N, L, d = 2, 5, 64
    e, cls, pos, gam, bet = n(N * (L - 1), d), n(d), n(L, d), 1 + 0.1 * n(d), 0.1 * n(d)
    ln = lambda s: TR.layer_norm(s.double(), gam.double(), bet.double()).float()      # noqa: E731
    rows = torch.cat([cls.expand(N, 1, d), e.view(N, L - 1, d)], 1)
    R.check_embed("right", ln(rows + pos).view(N * L, d), e, cls, pos, gam, bet)
    with pytest.raises(AssertionError):                                               # a missing class row
        R.check_embed("no class row", ln(e.view(N, L - 1, d) + pos[1:]).view(N * (L - 1), d), e, cls, pos, gam, bet)
    no_cls = torch.cat([e.view(N, L - 1, d)[:, :1], e.view(N, L - 1, d)], 1)          # ... or a patch row in its place
    with pytest.raises(AssertionError):
        R.check_embed("patch row for class row", ln(no_cls + pos).view(N * L, d), e, cls, pos, gam, bet)
    with pytest.raises(AssertionError):                                               # positions shifted by one row
        R.check_embed("shifted positions", ln(rows + pos.roll(1, 0)).view(N * L, d), e, cls, pos, gam, bet)
    x = n(N * L, d)
    R.check_pool("right", ln(x.view(N, L, d)[:, 0]), x, L, gam, bet)
    with pytest.raises(AssertionError):                                               # ln_post applied to row 1
        R.check_pool("row 1", ln(x.view(N, L, d)[:, 1]), x, L, gam, bet)
