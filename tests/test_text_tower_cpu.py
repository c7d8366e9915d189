"""The CLIP text tower without a GPU: the fp64 restatement (tests/text_tower_ref.py) against transformers' module and against the
recorded fixture (tests/golden/text_tower.npz, tools/make_golden_text_tower.py), the two key conventions, the first-maximum rule, every
refusal of the loader and of the Python surface, and the argument codes of the new entry points."""
import ctypes

import pytest
import torch

import matching_ref as MR
import text_tower_ref as R
from helpers import build_model, load_golden

F64 = torch.float64
EOTS = (3, 9, 20, 63, 12)


def golden():
    z = load_golden("text_tower.npz")
    sd = {k[2:]: torch.from_numpy(z[k]).to(F64) * float(z["scale/" + k[2:]]) for k in z.files if k.startswith("q/")}
    return sd, torch.from_numpy(z["ids"]), torch.from_numpy(z["out"]), int(z["heads"]), torch.from_numpy(z["eot"])


def maxrel(a, b):
    return float((a - b).abs().max() / b.abs().max())


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [77, 64])
def test_restatement_reproduces_the_fixture(L):
    """The recorded outputs are transformers' own (fp64, 77 positions); the restatement at 77 positions and trimmed to 64 -- an EOT sits
    at index 63 -- must agree to 1e-12: the trim is exact."""
    sd, ids, out, H, eot = golden()
    assert eot.tolist() == list(EOTS) and R.first_argmax(ids).tolist() == list(EOTS)
    assert maxrel(R.tower(sd, ids, H, L=L), out) <= 1e-12


@pytest.mark.parametrize("L", [77, 64])
def test_restatement_against_transformers(L):
    tr = pytest.importorskip("transformers")
    sd, ids, out, H, _ = golden()
    cfg = tr.CLIPTextConfig(vocab_size=300, hidden_size=64, intermediate_size=256, num_hidden_layers=3, num_attention_heads=H,
                            max_position_embeddings=77, projection_dim=48, hidden_act="quick_gelu", eos_token_id=2, bos_token_id=0,
                            pad_token_id=1)
    m = tr.CLIPTextModelWithProjection(cfg).double().eval()
    m.load_state_dict(sd, strict=False)
    with torch.no_grad():
        ref = m(input_ids=ids).text_embeds
    assert maxrel(ref, out) <= 1e-12                       # the fixture is what the module computes today
    assert maxrel(R.tower(sd, ids, H, L=L), ref) <= 1e-12


def test_key_conventions_give_identical_outputs():
    """OpenAI keys -> transformers keys (the reference file's converter) -> the package's canonical form -> both conventions again:
    the restatement's output is bit-identical through every hop, and so are the package's two exports."""
    from vct_amd import text as T
    oa = R.random_state_dict(64, 4, 256, 2, 48, 300, seed=3)
    hf = R.openai_to_transformers(oa)
    ids = R.caption_ids(EOTS, 300, seed=4)
    a = R.tower(oa, ids, 4)
    assert torch.equal(a, R.tower(hf, ids, 4))
    cw_oa, cw_hf = T.canonical_weights(oa), T.canonical_weights(hf)
    assert torch.equal(a, R.tower(T.to_openai_keys(cw_hf), ids, 4)) and torch.equal(a, R.tower(T.to_transformers_keys(cw_oa), ids, 4))
    for k in ("tok", "pos", "lnf_g", "lnf_b", "proj"):
        assert torch.equal(cw_oa[k], cw_hf[k]), k
    for la, lb in zip(cw_oa["layers"], cw_hf["layers"]):
        assert all(torch.equal(la[k], lb[k]) for k in la)
    assert not any(k.startswith("visual") or k == "logit_scale" for k in T.to_openai_keys(cw_oa))
    # fp16 weights (what clip.load leaves on a GPU) convert exactly
    half = {k: v.half() for k, v in oa.items()}
    assert torch.equal(T.canonical_weights(half)["tok"], oa["token_embedding.weight"].half().float())


def test_first_maximum_wins_when_the_largest_id_occurs_twice():
    from vct_amd import text as T
    ids = R.caption_ids((5, 2, 7), 300, seed=1, width=20)
    ids[0, 9] = 299                                         # a second EOT behind the first
    ids[2, 3] = 299                                         # ... and one in front of the original
    assert R.first_argmax(ids).tolist() == [5, 2, 3] == T.eot_positions(ids).tolist()
    assert T.eot_positions(ids.to(torch.int32)).tolist() == [5, 2, 3]
    assert T.trim_length(ids) == 6
    sd = R.random_state_dict(64, 4, 128, 1, 16, 300, seed=2)
    full, cut = R.tower(sd, ids, 4), R.tower(sd, ids, 4, L=6)
    assert maxrel(cut, full) <= 1e-12
    moved = ids.clone(); moved[0, 5] = 17                   # without the first EOT the pooled row moves to index 9
    assert maxrel(R.tower(sd, moved, 4)[0], full[0]) > 1e-3


def test_emulation_rounds_and_stays_close():
    """The bf16-rounding switch changes the result (it is on) by far less than SURVEY 8(d)'s 3e-2 at these shapes."""
    sd = R.random_state_dict(64, 4, 256, 2, 48, 300, seed=5)
    ids = R.caption_ids(EOTS, 300, seed=6)
    a, b = R.tower(sd, ids, 4, L=64), R.tower(sd, ids, 4, L=64, emulate=True)
    err = float((a - b).norm() / a.norm())
    assert 1e-4 < err < 3e-2, err


# ---- the loader and the Python surface --------------------------------------------------------------------------------------------------
def test_loader_reads_shapes_and_refuses_bad_dicts(tmp_path):
    from vct_amd.text import ClipTextTower
    oa = R.random_state_dict(64, 4, 256, 2, 48, 300, seed=3)
    t = ClipTextTower.from_state_dict(oa, "cpu", torch.float32, heads=4)
    assert (t.width, t.heads, t.layers, t.ff, t.dim, t.vocab) == (64, 4, 2, 256, 48, 300)
    assert ClipTextTower.from_state_dict(oa, "cpu", torch.float32).heads == 1          # CLIP's own rule: W // 64
    t16 = ClipTextTower.from_state_dict(R.openai_to_transformers(oa), "cpu", heads=4)
    assert t16.lw[0]["w_qkv"].dtype == torch.bfloat16 and t16.tok.dtype == t16.lw[0]["ln1_g"].dtype == t16.lw[0]["b_qkv"].dtype == torch.float32
    assert torch.equal(t16.lw[1]["w_fc"], oa["transformer.resblocks.1.mlp.c_fc.weight"].to(torch.bfloat16))
    assert torch.equal(t16.proj.float(), oa["text_projection"].t().to(torch.bfloat16).float())
    path = tmp_path / "clip.pt"
    torch.save(oa, path)
    assert ClipTextTower.from_file(str(path), "cpu", torch.float32, heads=4).dim == 48
    for conv in ("openai", "transformers"):
        sd = oa if conv == "openai" else R.openai_to_transformers(oa)
        for key in list(sd):
            if key.startswith("visual") or key == "logit_scale":
                continue
            with pytest.raises(ValueError, match=key.replace(".", r"\.")):
                ClipTextTower.from_state_dict({k: v for k, v in sd.items() if k != key}, "cpu", heads=4)
        key = [k for k in sd if k.endswith("out_proj.weight")][0]
        with pytest.raises(ValueError, match="out_proj"):
            ClipTextTower.from_state_dict({**sd, key: sd[key][:, :60]}, "cpu", heads=4)
    with pytest.raises(ValueError, match="token_embedding"):
        ClipTextTower.from_state_dict({"x": torch.zeros(1)}, "cpu")
    with pytest.raises(ValueError, match="heads"):
        ClipTextTower.from_state_dict(oa, "cpu", heads=3)                              # 64 % 3
    with pytest.raises(ValueError, match="compute_dtype"):
        ClipTextTower.from_state_dict(oa, "cpu", torch.float16, heads=4)


def test_python_refusals_before_any_device_work():
    from vct_amd.text import ClipTextTower
    t = ClipTextTower.from_state_dict(R.random_state_dict(64, 4, 128, 1, 48, 300, seed=3), "cpu", torch.float32, heads=4)
    ids = R.caption_ids((3, 64, 7), 300, seed=1)
    with pytest.raises(ValueError, match=r"caption 1 .*position 64.*at most 64"):
        t.encode_ids(ids)
    with pytest.raises(ValueError, match="at most 64"):
        t.encode_all(ids, chunk=2)
    with pytest.raises(RuntimeError, match="tokeniz"):
        t(["a man is cooking"])
    for bad in (ids.float(), ids[0], torch.zeros(2, 78, dtype=torch.int64), [[1, 2]]):
        with pytest.raises(ValueError, match="ids must be"):
            t.encode_ids(bad)
    with pytest.raises(ValueError, match="out must be"):
        t.encode_ids(ids[:1], out=torch.zeros(1, 47))


def _model(text_dim=48, **extra):
    mc = MR.matching_config([48], text_dim, MR.matching_block("CSL", "fixed", 0.5))
    mc.update(extra)
    return build_model(mc, 131, "cpu", torch.float32, MR.matching_params(mc, 131, 5))


def test_model_has_no_backend_until_a_tower_is_installed(tmp_path):
    from vct_amd.text import ClipTextTower
    oa = R.random_state_dict(64, 4, 128, 1, 48, 300, seed=3)
    m = _model()
    assert m.text_encoder.backend is None
    keys = set(m.state_dict())
    t = ClipTextTower.from_state_dict(oa, "cpu", torch.float32, heads=4)
    assert m.install_text_encoder(t) is t and m.text_encoder.backend is t
    assert set(m.state_dict()) == keys and not any(p is t.tok for p in m.parameters())       # frozen, outside the module
    with pytest.raises(ValueError, match="48.*64|64.*48"):
        _model(text_dim=64).install_text_encoder(t)
    assert _model(text_dim=64).text_encoder.backend is None
    t.device = torch.device("meta")
    with pytest.raises(ValueError, match="meta"):
        _model().install_text_encoder(t)
    # the optional config key: installed at construction, still without a tokenizer
    path = tmp_path / "clip.pt"
    torch.save({k: v for k, v in R.random_state_dict(64, 1, 128, 1, 48, 300, seed=3).items()}, path)
    m2 = _model(text_enc_weights=str(path))
    assert isinstance(m2.text_encoder.backend, ClipTextTower) and m2.text_encoder.backend.tokenize is None
    assert m2.text_encoder.backend.compute_dtype == torch.float32 and set(m2.state_dict()) == keys
    with pytest.raises(RuntimeError, match="tokeniz"):
        m2.text_encoder(["a caption"])


# ---- the C entry points -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from vct_amd import _lib
    return _lib.load()


def test_entry_points_validate_arguments(lib):
    """Codes, before any device use (there is no device here): the pointers are never dereferenced."""
    from vct_amd import _lib
    assert _lib.ACT["quick_gelu"] == 3 and lib.vct_abi_version() == 16
    p = ctypes.c_void_p
    a16, a8, a4 = p(4096), p(4096 + 8), p(4096 + 4)
    ok = (a16, a16, a16, a16)
    assert lib.vct_preln_fwd(1, 5, 64, None, a16, a16, a16, None) == -1
    assert lib.vct_preln_fwd(1, 5, 64, a16, None, a16, a16, None) == -1
    assert lib.vct_preln_fwd(1, 5, 64, a16, a16, None, a16, None) == -1
    assert lib.vct_preln_fwd(1, 5, 64, a16, a16, a16, None, None) == -1
    assert lib.vct_preln_fwd(2, 5, 64, *ok, None) == -1                      # bad dtype
    assert lib.vct_preln_fwd(1, 5, 1028, *ok, None) == -2                    # d > 1024
    assert lib.vct_preln_fwd(1, 5, 66, *ok, None) == -3                      # d % 4
    assert lib.vct_preln_fwd(1, 0, 64, *ok, None) == -2
    assert lib.vct_preln_fwd(0, 5, 64, a16, a16, a16, a8, None) == -3        # an fp32 y needs 16 bytes ...
    assert lib.vct_preln_fwd(1, 5, 64, a16, a16, a16, a4, None) == -3        # ... a bf16 y 8
    assert lib.vct_preln_fwd(1, 5, 64, a8, a16, a16, a16, None) == -3
    pool = lambda dt, B, L, Lids, d, ld, *ptrs: lib.vct_text_pool(dt, B, L, Lids, d, ptrs[0], ld, *ptrs[1:], None)      # noqa: E731
    good = [a16] * 7                                                         # ids, x, gamma, beta, y, eot, err
    for i in range(7):
        assert pool(1, 2, 8, 8, 64, 8, *[None if j == i else q for j, q in enumerate(good)]) == -1
    assert pool(3, 2, 8, 8, 64, 8, *good) == -1
    assert pool(1, 2, 8, 8, 1028, 8, *good) == -2 and pool(1, 2, 8, 8, 66, 8, *good) == -3
    assert pool(1, 0, 8, 8, 64, 8, *good) == -2 and pool(1, 2, 0, 8, 64, 8, *good) == -2
    assert pool(1, 2, 9, 8, 64, 8, *good) == -2 and pool(1, 2, 8, 8, 64, 7, *good) == -2      # Lids < L, ld_ids < Lids
    assert pool(1, 2, 8, 8, 64, 8, a4, *good[1:]) == -3                      # ids: 8 bytes
    assert pool(0, 2, 8, 8, 64, 8, *good[:4], a8, a16, a16) == -3
    # the new activation is forward only
    d = _lib.GemmDesc()
    d.dtype, d.out_dtype, d.tb, d.M, d.N, d.K, d.lda, d.ldb, d.ldc = 1, 1, 1, 8, 8, 8, 8, 8, 8
    d.A = d.B = d.C = d.dact_src = 4096
    d.ld_dact, d.act = 8, 3
    assert lib.vct_gemm(d, None) == -1
    d.dact_src, d.tb = None, 0                                               # ... and of the nn.Linear (NT) form only
    assert lib.vct_gemm(d, None) == -1
    d.tb, d.ta = 0, 1
    assert lib.vct_gemm(d, None) == -1


def test_python_wrappers_check_shapes():
    from vct_amd import ops
    x = torch.zeros(4, 64)
    with pytest.raises(AssertionError):
        ops.preln_fwd(x.double(), torch.ones(64), torch.zeros(64), torch.zeros(4, 64))
    with pytest.raises(AssertionError):
        ops.text_pool(torch.zeros(2, 2, dtype=torch.int32), x, 2, torch.ones(64), torch.zeros(64), torch.zeros(2, 64),
                      torch.zeros(2, dtype=torch.int32), torch.zeros(1, dtype=torch.int32))
