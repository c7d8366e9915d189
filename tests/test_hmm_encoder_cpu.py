"""The hierarchical multi-modal encoder (video_encoder.type "hmme") without a GPU: construction and state-dict surface against the
reference's recorded keys (tests/golden/hmm_state_keys.json), the per-layer routing table, the constructor's argument errors, the
gradient buckets over the new key names -- with the default `mme` model's flat layout pinned to the literal values of the commit
before this encoder existed -- and the argument errors of the vct_hmm_mix_* entry points."""
import json
import os

import numpy as np
import pytest
import torch

from encvar_ref import encvar_config
from helpers import GOLDEN, build_model
from hmm_ref import hmm_config, hmm_params, take_table

ENC = "video_encoder."
OPTS = dict(aggregation="max", temporal="embedding", do_norm=True)

# MMT4Caption(encvar_config([48, 24])): grad_buckets(), _ps.total and _ps.offsets in _ps.names order, recorded from the parent commit
PARENT_BUCKETS = [(0, 8576), (8576, 58944), (58944, 109184), (109184, 117568), (117568, 151168), (151168, 222912)]
PARENT_TOTAL = 222912
PARENT_OFFSETS = [
    ("cap_decoder.generator.weight", 0), ("cap_decoder.generator.bias", 8384), ("cap_decoder.decoder.norm.weight", 8576),
    ("cap_decoder.decoder.norm.bias", 8640), ("cap_decoder.decoder.layers.1.norm3.weight", 8704), ("cap_decoder.decoder.layers.1.norm3.bias", 8768),
    ("cap_decoder.decoder.layers.1.linear2.weight", 8832), ("cap_decoder.decoder.layers.1.linear2.bias", 17024),
    ("cap_decoder.decoder.layers.1.linear1.weight", 17088), ("cap_decoder.decoder.layers.1.linear1.bias", 25280),
    ("cap_decoder.decoder.layers.1.norm2.weight", 25408), ("cap_decoder.decoder.layers.1.norm2.bias", 25472),
    ("cap_decoder.decoder.layers.1.multihead_attn.out_proj.weight", 25536), ("cap_decoder.decoder.layers.1.multihead_attn.out_proj.bias", 29632),
    ("cap_decoder.decoder.layers.1.multihead_attn.in_proj_weight", 29696), ("cap_decoder.decoder.layers.1.multihead_attn.in_proj_bias", 41984),
    ("cap_decoder.decoder.layers.1.norm1.weight", 42176), ("cap_decoder.decoder.layers.1.norm1.bias", 42240),
    ("cap_decoder.decoder.layers.1.self_attn.out_proj.weight", 42304), ("cap_decoder.decoder.layers.1.self_attn.out_proj.bias", 46400),
    ("cap_decoder.decoder.layers.1.self_attn.in_proj_weight", 46464), ("cap_decoder.decoder.layers.1.self_attn.in_proj_bias", 58752),
    ("cap_decoder.decoder.layers.0.norm3.weight", 58944), ("cap_decoder.decoder.layers.0.norm3.bias", 59008),
    ("cap_decoder.decoder.layers.0.linear2.weight", 59072), ("cap_decoder.decoder.layers.0.linear2.bias", 67264),
    ("cap_decoder.decoder.layers.0.linear1.weight", 67328), ("cap_decoder.decoder.layers.0.linear1.bias", 75520),
    ("cap_decoder.decoder.layers.0.norm2.weight", 75648), ("cap_decoder.decoder.layers.0.norm2.bias", 75712),
    ("cap_decoder.decoder.layers.0.multihead_attn.out_proj.weight", 75776), ("cap_decoder.decoder.layers.0.multihead_attn.out_proj.bias", 79872),
    ("cap_decoder.decoder.layers.0.multihead_attn.in_proj_weight", 79936), ("cap_decoder.decoder.layers.0.multihead_attn.in_proj_bias", 92224),
    ("cap_decoder.decoder.layers.0.norm1.weight", 92416), ("cap_decoder.decoder.layers.0.norm1.bias", 92480),
    ("cap_decoder.decoder.layers.0.self_attn.out_proj.weight", 92544), ("cap_decoder.decoder.layers.0.self_attn.out_proj.bias", 96640),
    ("cap_decoder.decoder.layers.0.self_attn.in_proj_weight", 96704), ("cap_decoder.decoder.layers.0.self_attn.in_proj_bias", 108992),
    ("cap_decoder.tgt_to_emb.weight", 109184), ("video_encoder.transformer_encoder.norm.weight", 117568), ("video_encoder.transformer_encoder.norm.bias",
    117632), ("video_encoder.transformer_encoder.layers.1.norm2.weight", 117696), ("video_encoder.transformer_encoder.layers.1.norm2.bias", 117760),
    ("video_encoder.transformer_encoder.layers.1.linear2.weight", 117824), ("video_encoder.transformer_encoder.layers.1.linear2.bias", 126016),
    ("video_encoder.transformer_encoder.layers.1.linear1.weight", 126080), ("video_encoder.transformer_encoder.layers.1.linear1.bias", 134272),
    ("video_encoder.transformer_encoder.layers.1.norm1.weight", 134400), ("video_encoder.transformer_encoder.layers.1.norm1.bias", 134464),
    ("video_encoder.transformer_encoder.layers.1.self_attn.out_proj.weight", 134528),
    ("video_encoder.transformer_encoder.layers.1.self_attn.out_proj.bias", 138624),
    ("video_encoder.transformer_encoder.layers.1.self_attn.in_proj_weight", 138688), ("video_encoder.transformer_encoder.layers.1.self_attn.in_proj_bias",
    150976), ("video_encoder.transformer_encoder.layers.0.norm2.weight", 151168), ("video_encoder.transformer_encoder.layers.0.norm2.bias", 151232),
    ("video_encoder.transformer_encoder.layers.0.linear2.weight", 151296), ("video_encoder.transformer_encoder.layers.0.linear2.bias", 159488),
    ("video_encoder.transformer_encoder.layers.0.linear1.weight", 159552), ("video_encoder.transformer_encoder.layers.0.linear1.bias", 167744),
    ("video_encoder.transformer_encoder.layers.0.norm1.weight", 167872), ("video_encoder.transformer_encoder.layers.0.norm1.bias", 167936),
    ("video_encoder.transformer_encoder.layers.0.self_attn.out_proj.weight", 168000),
    ("video_encoder.transformer_encoder.layers.0.self_attn.out_proj.bias", 172096),
    ("video_encoder.transformer_encoder.layers.0.self_attn.in_proj_weight", 172160), ("video_encoder.transformer_encoder.layers.0.self_attn.in_proj_bias",
    184448), ("video_encoder.unify.0.weight", 184640), ("video_encoder.unify.0.bias", 187712), ("video_encoder.unify.1.weight", 187776),
    ("video_encoder.unify.1.bias", 189312), ("video_encoder.modal_emb.modal_emb.weight", 189376), ("matching.v_proj.weight", 189632),
    ("matching.v_proj.bias", 222400)
]


@pytest.fixture(scope="module")
def ref_keys():
    with open(os.path.join(GOLDEN, "hmm_state_keys.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("tag,opts", [("default", {}), ("options", OPTS)])
@pytest.mark.parametrize("shapes,layers", [([48, 24], [2, 1]), ([48, 24], [1, 3]), ([48], [2])])
def test_constructs_with_the_reference_state_dict(ref_keys, shapes, layers, tag, opts):
    mc = hmm_config(shapes, layers, **opts)
    m = build_model(mc, 131, "cpu", torch.float32, hmm_params(mc, 131, 5))      # (asserts: nothing unexpected, only matching.* missing)
    want = dict(ref_keys["rest"], **ref_keys["encoder"][f"{layers}/{tag}"])
    sd = m.state_dict()
    assert sorted(k for k in sd if not k.startswith("matching.")) == sorted(k for k in want if not k.startswith("matching."))
    for k, shp in want.items():
        if not k.startswith("matching."):
            assert list(sd[k].shape) == shp, k
    assert not any("transformer_encoder" in k for k in sd)
    L = max(layers)
    assert {int(k.split(".")[2]) for k in sd if k.startswith(ENC + "trans_enc_layers.")} == set(range(L))
    assert (ENC + "norm.weight" in sd) == bool(opts) and (ENC + "temp_emb.embedding.weight" in sd) == bool(opts)
    assert (ENC + "modal_emb.modal_emb.weight" in sd) == (len(shapes) > 1)
    assert m.video_encoder.cfg["layers"] == L and m.video_encoder.num_encoder_layers == layers


def test_layers_start_as_copies_of_one_layer():
    sd = build_model(hmm_config([48, 24], [1, 3]), 131, "cpu", torch.float32).state_dict()
    l0 = {k[len(ENC + "trans_enc_layers.0."):]: v for k, v in sd.items() if k.startswith(ENC + "trans_enc_layers.0.")}
    assert len(l0) == 12 and float(l0["linear1.weight"].abs().max()) > 0
    for l in (1, 2):
        for k, v in l0.items():
            assert torch.equal(sd[f"{ENC}trans_enc_layers.{l}.{k}"], v), (l, k)


@pytest.mark.parametrize("layers,Ts", [(l, t) for l in ([2, 1], [1, 3], [3, 1, 2], [2, 2], [4]) for t in ((5, 3), (4, 1, 2), (1, 1))
                                       if len(l) == len(t)] + [([4], (5,)), ([4], (1,))])
def test_take_table(layers, Ts):
    from vct_amd.engine import HMMEncoderEngine
    L, target = max(layers), [max(layers) - n for n in layers]
    want = np.zeros((L, sum(t + 1 for t in Ts)), np.uint8)      # the reference's rule: target[j] < i
    for i in range(L):
        at = 0
        for j, t in enumerate(Ts):
            want[i, at:at + t + 1] = target[j] < i
            at += t + 1
    got = HMMEncoderEngine.take_table(layers, Ts)
    assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want) and np.array_equal(take_table(layers, Ts), want)
    assert not got[0].any()                                     # layer 0 takes the stack input as it is
    assert got[max(target) + 1:].all()                          # above max(target) every row continues
    mixed = [i for i in range(L) if got[i].any() and not got[i].all()]
    assert all(1 <= i <= max(target) for i in mixed)
    if len(set(layers)) == 1:
        assert mixed == []                                      # equal depths: no mixed row, no launch
    if layers == [1, 3] and Ts == (5, 3):
        assert got.tolist() == [[0] * 10, [0] * 6 + [1] * 4, [0] * 6 + [1] * 4]


def test_take_table_is_built_once_per_frame_counts(monkeypatch):
    from vct_amd.engine import HMMEncoderEngine
    eng = build_model(hmm_config([48, 24], [1, 3]), 131, "cpu", torch.float32).video_encoder._engine()
    assert isinstance(eng, HMMEncoderEngine)
    calls = []
    orig = HMMEncoderEngine.take_table
    monkeypatch.setattr(HMMEncoderEngine, "take_table", staticmethod(lambda *a: (calls.append(a), orig(*a))[1]))
    take, top = eng.take_rows((5, 3))
    assert top == 2 and take.dtype == torch.uint8 and take.tolist() == take_table([1, 3], (5, 3)).tolist()
    assert eng.take_rows((5, 3))[0] is take and len(calls) == 1
    eng.take_rows((4, 2))
    assert len(calls) == 2
    with pytest.raises(ValueError):
        HMMEncoderEngine.take_table([1, 3], (5, 3, 2))


@pytest.mark.parametrize("layer", [2, [2], [2, 1, 1], [2, 0], [2, -1], [2, 1.0], [True, 2], None])
def test_layer_list_errors(layer):
    mc = hmm_config([48, 24], [2, 1])
    mc["video_encoder"]["layer"] = layer
    with pytest.raises(ValueError):
        build_model(mc, 131, "cpu", torch.float32)


def test_simple_and_gru_still_raise():
    mc = encvar_config([48, 24])
    mc["video_encoder"]["type"] = "simple"
    with pytest.raises(NotImplementedError):
        build_model(mc, 131, "cpu", torch.float32)
    for agg in ("GRU", "biGRU"):
        with pytest.raises(NotImplementedError):
            build_model(hmm_config([48, 24], [2, 1], aggregation=agg), 131, "cpu", torch.float32)


def test_config_check_accepts_hmme(tmp_path):
    from vct_amd.utils import Config
    for typ, ok in (("hmme", True), ("mme", True), ("simple", False)):
        mc = hmm_config([48, 24], [2, 1])
        mc["video_encoder"]["type"] = typ
        p = tmp_path / f"{typ}.json"
        p.write_text(json.dumps({"model": mc}))
        if ok:
            Config(str(p)).check()
        else:
            with pytest.raises(ValueError):
                Config(str(p)).check()


@pytest.mark.parametrize("shapes,layers,opts", [([48, 24], [2, 1], {}), ([48, 24], [1, 3], OPTS), ([48, 24, 16], [3, 1, 2], {}), ([48], [2], {})])
def test_grad_buckets_over_the_new_keys(shapes, layers, opts):
    m = build_model(hmm_config(shapes, layers, **opts), 131, "cpu", torch.float32)
    ps, b, L = m._ps, m.grad_buckets(), max(layers)
    assert b[0][0] == 0 and b[-1][1] == ps.total and all(b[i][1] == b[i + 1][0] and b[i][0] < b[i][1] for i in range(len(b) - 1))
    assert len(b) == 2 + 2 + L                  # generator | 2 decoder layers | embedding | L encoder layers
    named = dict(m.named_parameters())

    def bucket_of(n):
        hit = [i for i, (s, e) in enumerate(b) if s <= ps.offsets[n] and ps.offsets[n] + named[n].numel() <= e]
        assert len(hit) == 1, n
        return hit[0]
    seen = 0
    for n in ps.names:
        if n.startswith(ENC + "trans_enc_layers."):
            assert bucket_of(n) == m.bucket_index("enc_layer", int(n.split(".")[2])), n
            seen += 1
        elif n.startswith(ENC):                 # the front end: unify.*, modal_emb, temp_emb.embedding, norm
            assert bucket_of(n) == len(b) - 1 == m.bucket_index("enc_layer", 0), n
    assert seen == 12 * L
    assert m.encoder_param_begin == b[m.bucket_index("enc_layer", L - 1)][0] == ps.offsets[f"{ENC}trans_enc_layers.{L - 1}.norm2.weight"]
    assert all(named[n].data_ptr() == ps.flat.data_ptr() + 4 * ps.offsets[n] for n in ps.names)


def test_default_mme_flat_layout_is_the_parents():
    m = build_model(encvar_config([48, 24]), 131, "cpu", torch.float32)
    assert [tuple(x) for x in m.grad_buckets()] == PARENT_BUCKETS and m._ps.total == PARENT_TOTAL
    assert [(n, m._ps.offsets[n]) for n in m._ps.names] == PARENT_OFFSETS
    assert [m.bucket_index("enc_layer", l) for l in (1, 0)] == [4, 5]


def test_weight_file_round_trip(tmp_path):
    from vct_amd import checkpoint as ck
    mc = hmm_config([48, 24], [1, 3], **OPTS)
    p = hmm_params(mc, 131, 9)
    a = build_model(mc, 131, "cpu", torch.float32, p)
    ck.save_weights(a, str(tmp_path / "w.pt"))
    b = build_model(mc, 131, "cpu", torch.float32)
    ck.load_weights(b, str(tmp_path / "w.pt"))
    sd = b.state_dict()
    for k, v in p.items():
        assert np.array_equal(sd[k].numpy(), v), k
    assert b._ps.intact()
    assert not np.array_equal(p[ENC + "trans_enc_layers.0.linear1.weight"], p[ENC + "trans_enc_layers.2.linear1.weight"])   # hmm_ref: per-layer values


def test_mix_entry_points_reject_bad_arguments():
    import __graft_entry__ as g
    g.build()
    from vct_amd import _lib
    lib = _lib.load()
    assert "vct_hmm_mix_fwd" in _lib.exported_symbols() and "vct_hmm_mix_bwd" in _lib.exported_symbols()
    assert lib.vct_hmm_mix_fwd(None, None) == -1 and lib.vct_hmm_mix_bwd(None, None) == -1      # null descriptor
    A = 4096                                                      # an aligned non-null address: nothing is dereferenced on these paths

    def desc(**kw):
        d = _lib.HmmMixDesc()
        d.dtype, d.B, d.S, d.d = 0, 2, 7, 64
        d.take, d.y, d.x0, d.x, d.dx, d.dy, d.acc = A, A, A, A, A, A, A
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    for fn in (lib.vct_hmm_mix_fwd, lib.vct_hmm_mix_bwd):
        assert fn(desc(dtype=5), None) == -1                      # bad dtype
        assert fn(desc(S=0), None) == -2 and fn(desc(S=1025), None) == -2 and fn(desc(B=0), None) == -2 and fn(desc(d=0), None) == -2
        assert fn(desc(d=66), None) == -3 and fn(desc(dtype=1, d=68), None) == -3       # width not a multiple of the vector
        assert fn(desc(take=None), None) == -1
    for k in ("y", "x0", "x"):
        assert lib.vct_hmm_mix_fwd(desc(**{k: None}), None) == -1
        assert lib.vct_hmm_mix_fwd(desc(**{k: A + 4}), None) == -3
    for k in ("dx", "dy", "acc"):
        assert lib.vct_hmm_mix_bwd(desc(**{k: None}), None) == -1
        assert lib.vct_hmm_mix_bwd(desc(**{k: A + 8}), None) == -3
    assert lib.vct_hmm_mix_bwd(desc(dx0=A, acc=None, dy=None, take=None), None) == -1      # the layer-0 form still reads the accumulator
    assert lib.vct_hmm_mix_bwd(desc(dx0=A, init=1, dy=None, take=None), None) == -1        # ... which an earlier launch initialised
    assert lib.vct_hmm_mix_bwd(desc(dx0=A + 4, dy=None, take=None), None) == -3            # dy / take are not needed there
