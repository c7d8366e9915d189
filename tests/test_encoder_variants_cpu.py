"""The encoder's option surface without a GPU (temporal 'embedding', aggregation 'max', do_norm; tests/golden/encvar_*): construction
and state-dict surface of all eight combinations against the reference's recorded keys, the flat-buffer place of the new parameters,
the temporal index table, and the argument errors of the vct_enc_frontend_ex_* entry points."""
import json
import os

import numpy as np
import pytest
import torch

from encvar_ref import COMBOS, combo_key, encvar_config, encvar_params, temporal_index
from helpers import GOLDEN, build_model, load_golden, model_config_of

ENC = "video_encoder."
NEW = {"embedding": [ENC + "temp_emb.embedding.weight"], "norm": [ENC + "norm.weight", ENC + "norm.bias"]}


@pytest.fixture(scope="module")
def ref_keys():
    """The reference's state_dict keys -> shapes per combination: the fixture holds the default's per stream count and what each
    combination adds to / drops from it."""
    with open(os.path.join(GOLDEN, "encvar_state_keys.json")) as f:
        z = json.load(f)
    out = {}
    for key, diff in z["combos"].items():
        keys = dict(z["default"][key.split("/")[0]])
        for k in diff["drop"]:
            del keys[k]
        keys.update(diff["add"])
        out[key] = keys
    return out


@pytest.mark.parametrize("shapes", [[48], [48, 24]])
@pytest.mark.parametrize("agg,temporal,norm", COMBOS)
def test_every_combination_constructs_with_the_reference_state_dict(ref_keys, shapes, agg, temporal, norm):
    mc = encvar_config(shapes, agg, temporal, norm)
    m = build_model(mc, 131, "cpu", torch.float32, encvar_params(mc, 131, 5))      # (asserts: nothing unexpected, only matching.* missing)
    want = ref_keys[combo_key(len(shapes), agg, temporal, norm)]
    sd = m.state_dict()
    assert sorted(k for k in sd if not k.startswith("matching.")) == sorted(want)
    for k, shp in want.items():
        assert list(sd[k].shape) == shp, k
    assert (ENC + "temp_emb.pe" in sd) == (temporal == "encoding")
    assert (ENC + "temp_emb.embedding.weight" in sd) == (temporal == "embedding")
    assert (ENC + "norm.weight" in sd) == bool(norm)
    fresh = build_model(mc, 131, "cpu", torch.float32).state_dict()
    if temporal == "embedding":
        assert want[ENC + "temp_emb.embedding.weight"] == [512, 64]
        assert 0.9 < float(fresh[ENC + "temp_emb.embedding.weight"].std()) < 1.1          # nn.Embedding's N(0, 1)
    if norm:
        assert torch.equal(fresh[ENC + "norm.weight"], torch.ones(64)) and torch.equal(fresh[ENC + "norm.bias"], torch.zeros(64))


@pytest.mark.parametrize("case", ["E", "M", "N", "X", "S"])
def test_fixture_state_keys(case):
    z = load_golden(f"encvar_{case}.npz")
    mc = model_config_of(z)
    m = build_model(mc, int(z["vocab"]), "cpu", torch.float32, encvar_params(mc, int(z["vocab"]), int(z["param_seed"])))
    keys = json.loads(str(z["state_keys"]))
    sd = m.state_dict()
    assert sorted(k for k in sd if not k.startswith("matching.")) == sorted(keys)
    assert all(list(sd[k].shape) == shp for k, shp in keys.items())


def test_default_constructor_arguments_build_the_learned_table():
    """The reference's (and our) constructor default is temporal_type 'embedding': MultiModalEncoder([512], 512, 8) must construct."""
    from vct_amd.model.MMEncoder import MultiModalEncoder
    enc = MultiModalEncoder([64], 64, 4, dim_feedforward=128, num_encoder_layers=1, device=torch.device("cpu"),
                            compute_dtype=torch.float32)
    assert tuple(enc.temp_emb.embedding.weight.shape) == (512, 64) and not hasattr(enc.temp_emb, "pe")


@pytest.mark.parametrize("agg", ["GRU", "biGRU"])
def test_gru_aggregations_still_raise(agg):
    with pytest.raises(NotImplementedError):
        build_model(encvar_config([48, 24], agg), 131, "cpu", torch.float32)


@pytest.mark.parametrize("Ts", [(5, 3), (5,), (12, 8, 3), (1, 1)])
def test_temporal_index_table(Ts):
    from vct_amd.engine import EncoderEngine
    want = np.concatenate([np.concatenate([[0], np.linspace(1, Ts[0], t).astype(np.int32)]) for t in Ts])
    got = EncoderEngine.temporal_index(Ts)
    assert got.dtype == np.int32 and np.array_equal(got, want) and np.array_equal(temporal_index(Ts), want)
    if Ts == (5, 3):
        assert got.tolist() == [0, 1, 2, 3, 4, 5, 0, 1, 3, 5]
    mc = encvar_config([48, 24][:len(Ts)] if len(Ts) <= 2 else [48, 24, 16], temporal="embedding")
    enc = build_model(mc, 131, "cpu", torch.float32).video_encoder._engine()
    rows = enc.ex_rows(Ts)
    assert rows["tidx"].dtype == torch.int32 and rows["tidx"].tolist() == want.tolist() and "temp" not in rows
    assert (rows["labels"] is None) == (len(Ts) == 1)
    assert enc.ex_rows(Ts) is rows                  # built once per frame-count tuple
    with pytest.raises(ValueError):
        enc.ex_rows((512,) + Ts[1:])                # frame 512 of the first stream would read row 512 of 512


@pytest.mark.parametrize("shapes", [[48], [48, 24]])
def test_new_parameters_sit_in_the_last_bucket_inside_the_caption_range(shapes):
    m = build_model(encvar_config(shapes, "max", "embedding", True), 131, "cpu", torch.float32)
    ps = m._ps
    new = NEW["embedding"] + NEW["norm"]
    b = m.grad_buckets()
    assert b[0][0] == 0 and b[-1][1] == ps.total and all(b[i][1] == b[i + 1][0] for i in range(len(b) - 1))
    last = b[m.bucket_index("enc_layer", 0)]
    assert last == b[-1]
    after = ENC + ("modal_emb.modal_emb.weight" if len(shapes) > 1 else "unify.0.bias")
    at = ps.names.index(after)
    assert ps.names[at + 1:at + 1 + len(new)] == new          # named explicitly, behind unify.* / modal_emb ...
    assert ps.names[at + 1 + len(new)].startswith("matching.")      # ... and in front of what the caption task does not own
    named = dict(m.named_parameters())
    for n in new:
        assert m.encoder_param_begin <= ps.offsets[n] and ps.offsets[n] + named[n].numel() <= m.caption_param_end, n
        assert last[0] <= ps.offsets[n] < last[1], n
        assert named[n].data_ptr() == ps.flat.data_ptr() + 4 * ps.offsets[n]


def test_weight_file_round_trip(tmp_path):
    from vct_amd import checkpoint as ck
    mc = encvar_config([48, 24], "max", "embedding", True)
    p = encvar_params(mc, 131, 9)
    a = build_model(mc, 131, "cpu", torch.float32, p)
    ck.save_weights(a, str(tmp_path / "w.pt"))
    b = build_model(mc, 131, "cpu", torch.float32)
    ck.load_weights(b, str(tmp_path / "w.pt"))
    for k in NEW["embedding"] + NEW["norm"]:
        assert np.array_equal(b.state_dict()[k].numpy(), p[k]), k
    assert b._ps.intact()


def test_ex_entry_points_reject_bad_arguments():
    import __graft_entry__ as g
    g.build()
    from vct_amd import _lib
    lib = _lib.load()
    assert "vct_enc_frontend_ex_fwd" in _lib.exported_symbols() and "vct_enc_frontend_ex_bwd" in _lib.exported_symbols()
    assert lib.vct_enc_frontend_ex_fwd(None, None) == -1          # null descriptor
    assert lib.vct_enc_frontend_ex_bwd(None, None) == -1
    A = 4096                                                      # an aligned non-null address: nothing is dereferenced on these paths

    def desc(**kw):
        d = _lib.EncFrontendExDesc()
        d.dtype, d.n, d.B, d.d, d.n_labels = 0, 2, 2, 64, 4
        d.T[0], d.T[1] = 3, 2
        for i in range(2):
            d.u[i], d.du[i] = A, A
        d.temp, d.modal_w, d.labels, d.x0, d.dx, d.d_modal = A, A, A, A, A, A
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    for fn in (lib.vct_enc_frontend_ex_fwd, lib.vct_enc_frontend_ex_bwd):
        assert fn(desc(dtype=5), None) == -1                      # bad dtype
        assert fn(desc(agg=2), None) == -1 and fn(desc(temporal=3), None) == -1
        assert fn(desc(n=0), None) == -2                          # no stream
        assert fn(desc(n=_lib.MM_MAX_MODAL + 1), None) == -2
        assert fn(desc(n_labels=3), None) == -2                   # label rows must be n or 2n
        assert fn(desc(d=2048), None) == -2                       # a row no longer fits one wave's registers
        assert fn(desc(d=66), None) == -3                         # width not a multiple of the vector
        assert fn(desc(dtype=1, d=68), None) == -3
        assert fn(desc(temporal=1, emb_rows=512, tidx=A), None) == -1       # learned: no weight (fwd) / no d_emb (bwd)
        assert fn(desc(temporal=1, emb_rows=512, emb_w=A), None) == -1                     # learned: no index table
        assert fn(desc(temporal=1, emb_rows=0, emb_w=A, tidx=A), None) == -2
        assert fn(desc(norm=1, gamma=A, beta=A), None) == -1      # the norm without its row statistics
        assert fn(desc(norm=1, mean=A, rstd=A), None) == -1       # ... without its weight
        assert fn(desc(p_drop=1.0), None) == -1
        d = desc()
        d.T[1] = 0
        assert fn(d, None) == -2                                  # empty stream
        d.T[1] = 2000
        assert fn(d, None) == -2                                  # S > 1024
    assert lib.vct_enc_frontend_ex_fwd(desc(temp=None), None) == -1
    assert lib.vct_enc_frontend_ex_fwd(desc(x0=None), None) == -1
    assert lib.vct_enc_frontend_ex_fwd(desc(x0=A + 4), None) == -3
    # one stream needs no modal table: the checks run on to the (misaligned) output
    assert lib.vct_enc_frontend_ex_fwd(desc(n=1, labels=None, modal_w=None, n_labels=0, x0=A + 4), None) == -3
    assert lib.vct_enc_frontend_ex_bwd(desc(dx=None), None) == -1
    assert lib.vct_enc_frontend_ex_bwd(desc(dx=A + 8), None) == -3
    assert lib.vct_enc_frontend_ex_bwd(desc(d_modal=None), None) == -1
    assert lib.vct_enc_frontend_ex_bwd(desc(agg=1, u=(_lib.vp * _lib.MM_MAX_MODAL)()), None) == -1       # 'max' recomputes the argmax from u
    # 'max' without the norm scans u alone: the temporal / modal tables are neither read nor required (the checks run on to dx)
    assert lib.vct_enc_frontend_ex_bwd(desc(agg=1, temp=None, modal_w=None, dx=A + 8), None) == -3
    assert lib.vct_enc_frontend_ex_bwd(desc(agg=1, temporal=1, emb_rows=512, tidx=A, d_emb=A, temp=None, modal_w=None, dx=A + 8), None) == -3
    assert lib.vct_enc_frontend_ex_bwd(desc(norm=1, gamma=A, mean=A, rstd=A, dpre=A, param_ws=A, temp=None), None) == -1   # the norm recomputes pre
    assert lib.vct_enc_frontend_ex_bwd(desc(norm=1, gamma=A, mean=A, rstd=A), None) == -1               # norm: no dpre / partials buffer
