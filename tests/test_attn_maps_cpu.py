"""Cross-attention maps, CPU side: the Vis decoder type constructs with the plain decoder's state_dict surface, the library exports
vct_attn_weights and validates its arguments without a device, the numpy reference of the GPU tests agrees with the reference
fixture, and beam search refuses return_attn before touching a device."""
import json

import numpy as np
import pytest
import torch

import vct_oracle as O
from attnmap_ref import attn_weights_ref
from helpers import build_model, load_golden, model_config_of


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from vct_amd import _lib
    return _lib.load()


def _fixture():
    z = load_golden("attnmap_train.npz")
    mc = model_config_of(z)
    V = int(z["vocab"])
    return z, mc, V, O.init_params(O.cfg_from_model_config(mc, V), seed=int(z["param_seed"]))


def test_vis_decoder_type_constructs_with_the_plain_state_dict():
    from vct_amd.model import CapDecoder
    z, mc, V, p = _fixture()
    assert mc["caption_decoder"]["layer_type"] == "vis"
    dec = CapDecoder(2, 64, 4, 128, 0.0, V, 0, 0.5, custom_decoder_type="vis", device=torch.device("cpu"), compute_dtype=torch.float32)
    ref = CapDecoder(2, 64, 4, 128, 0.0, V, 0, 0.5, device=torch.device("cpu"), compute_dtype=torch.float32)
    assert list(dec.state_dict()) == list(ref.state_dict())
    assert not hasattr(ref, "attn_weights") and not hasattr(dec, "attn_weights")       # set by a forward only
    m = build_model(mc, V, "cpu", torch.float32, p)                                    # (asserts: nothing unexpected, only matching.* missing)
    plain_mc = json.loads(json.dumps(mc))
    del plain_mc["caption_decoder"]["layer_type"]
    plain = build_model(plain_mc, V, "cpu", torch.float32)
    keys = json.loads(str(z["state_keys"]))
    sd = m.state_dict()
    assert list(sd) == list(plain.state_dict())
    assert sorted(k for k in sd if not k.startswith("matching.")) == sorted(keys)
    for k, shp in keys.items():
        assert list(sd[k].shape) == shp, k
    assert m.cap_decoder._engine().attn_maps and not plain.cap_decoder._engine().attn_maps


def test_library_exports_attn_weights(lib):
    from vct_amd import _lib
    assert "vct_attn_weights" in _lib.exported_symbols()
    assert hasattr(lib, "vct_attn_weights")


def test_attn_weights_argument_errors_are_codes(lib):
    """NULL pointers -> VCT_E_ARG, shapes beyond vct_attn_fwd's limits -> VCT_E_SHAPE, misaligned leading dimensions -> VCT_E_ALIGN,
    all without touching a device."""
    import ctypes
    from vct_amd import _lib
    assert lib.vct_attn_weights(None, None) == -1
    d = _lib.AttnWeightsDesc()
    d.dtype, d.B, d.H, d.Lq, d.Lk, d.hd = _lib.BF16, 2, 4, 6, 6, 16
    assert lib.vct_attn_weights(d, None) == -1                         # null operands
    buf = (ctypes.c_float * 64)()
    ptr = (ctypes.addressof(buf) + 15) // 16 * 16
    d.q = d.k = d.w = ptr
    d.ldq = d.ldk = 64
    d.ldw = 6
    d.dtype = 7
    assert lib.vct_attn_weights(d, None) == -1                         # bad dtype enum
    d.dtype = _lib.BF16
    d.Lk, d.ldw = 65, 65
    assert lib.vct_attn_weights(d, None) == -2
    d.Lk, d.ldw, d.hd = 6, 6, 136
    assert lib.vct_attn_weights(d, None) == -2
    d.hd, d.Lq = 16, 65
    assert lib.vct_attn_weights(d, None) == -2
    d.Lq, d.ldw = 6, 5
    assert lib.vct_attn_weights(d, None) == -2                         # output rows narrower than Lk
    d.ldw, d.ldq = 6, 60
    assert lib.vct_attn_weights(d, None) == -3                         # bf16 leading dimensions: multiples of 8
    d.ldq, d.hd = 64, 12
    assert lib.vct_attn_weights(d, None) == -3


def test_fixture_rows_sum_to_one_and_leave_comparable_decode_rows():
    z = load_golden("attnmap_train.npz")
    ids = z["ids"]
    for l in range(2):
        a = z[f"attn{l}"]
        assert a.shape == (3, ids.shape[1] - 1, z["feats"].shape[1] + 1) and a.dtype == np.float32
        assert np.abs(a.astype(np.float64).sum(-1) - 1.0).max() < 1e-6
    first_pad = [int(np.argmax(r == 0)) if (r == 0).any() else len(r) for r in ids[:, :-1]]
    assert first_pad == z["first_pad"].tolist() and min(first_pad) >= 4


def test_numpy_reference_agrees_with_the_fixture():
    """Layer 0's q and K projections in numpy, from the recorded memory and multihead_attn input and the seed's in_proj."""
    z, mc, V, p = _fixture()
    d, H = 64, 4
    pre = O.DEC + "decoder.layers.0.multihead_attn."
    w, b = p[pre + "in_proj_weight"].astype(np.float64), p[pre + "in_proj_bias"].astype(np.float64)
    q = z["act/ca_in0"].astype(np.float64) @ w[:d].T + b[:d]
    k = z["act/memory"].astype(np.float64) @ w[d:2 * d].T + b[d:2 * d]
    got = attn_weights_ref(q, k, H)
    assert np.abs(got - z["attn0"]).max() < 1e-6           # fp32 torch against fp64: a few fp32 ulps of values <= 1


def test_numpy_reference_masks():
    rng = np.random.default_rng(0)
    q, k = rng.standard_normal((2, 5, 8)), rng.standard_normal((2, 5, 8))
    w = attn_weights_ref(q, k, 2, causal=True)
    assert np.all(w[:, np.triu_indices(5, 1)[0], np.triu_indices(5, 1)[1]] == 0) and np.allclose(w.sum(-1), 1)
    kp = np.ones((2, 4), bool)
    kp[0, :2] = False
    w = attn_weights_ref(q, k, 2, key_pad=kp, shift=1)
    assert np.all(w[0, :, 3:] == 0) and np.all(w[1, :, 1:] == 0) and np.allclose(w.sum(-1), 1)
    w = attn_weights_ref(q, k, 2, key_pad=np.ones((2, 5), bool))
    assert np.all(w == 0)


def test_average_attention_is_the_mean_over_layers():
    from vct_amd.evaluate import average_attention
    z = load_golden("attnmap_train.npz")
    maps = torch.from_numpy(np.stack([z["attn0"], z["attn1"]], 1))            # [B, layers, steps, Te]
    want = np.stack([z["attn0"], z["attn1"]], 1).mean(1)
    assert np.allclose(average_attention(maps).numpy(), want, atol=1e-7)
    assert np.allclose(average_attention(maps[1], 3).numpy(), want[1, :3], atol=1e-7)
    with pytest.raises(ValueError):
        average_attention(maps[0, 0])


def test_beam_search_refuses_return_attn_before_any_device_work():
    from vct_amd import decode
    z, mc, V, p = _fixture()
    m = build_model(mc, V, "cpu", torch.float32, p)
    feats = torch.from_numpy(z["feats"])
    with pytest.raises(ValueError, match="beam"):
        m.beam_decode([feats], None, beam_size=2, max_len=6, return_attn=True)
    with pytest.raises(ValueError, match="beam"):
        m.beam_decode_ids([feats], None, beam_size=2, max_len=6, return_attn=True)
    with pytest.raises(ValueError, match="beam"):
        decode.beam_decode_ids(m, feats, None, 2, max_len=6, return_attn=True)
    with pytest.raises(ValueError, match="beam"):
        decode.beam_decode_ids_reference_algorithm(m, feats, None, 2, max_len=6, return_attn=True)
    from vct_amd import evaluate
    with pytest.raises(ValueError, match="beam"):
        evaluate.v2t_batch(m, [feats], None, max_len=6, beam_size=2, return_attn=True)
