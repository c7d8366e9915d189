"""Multi-modal video input without a GPU: state-dict surface against the reference's keys (tests/golden/mm_*.npz), the flat
parameter layout and gradient buckets with the new parameters, checkpoint round trips, and argument errors of the two
front-end entry points."""
import json

import numpy as np
import pytest
import torch

from helpers import build_model, load_golden, model_config_of
from mm_ref import mm_config, mm_params


@pytest.mark.parametrize("name", ["mm_train.npz", "mm_train3.npz"])
def test_state_keys_and_shapes_equal_reference(name):
    z = load_golden(name)
    mc = model_config_of(z)
    m = build_model(mc, int(z["vocab"]), "cpu", torch.float32)
    keys = json.loads(str(z["state_keys"]))
    sd = m.state_dict()
    assert sorted(k for k in sd if not k.startswith("matching.")) == sorted(keys)
    for k, shp in keys.items():
        assert list(sd[k].shape) == shp, k
    n = len(mc["modal_shape"])
    rows = 2 * n if mc["video_encoder"]["mme"]["modal_different"] else n
    assert keys["video_encoder.modal_emb.modal_emb.weight"] == [rows, mc["embed_dim"]]
    w = sd["video_encoder.modal_emb.modal_emb.weight"]
    assert 0.5 < float(w.std()) < 1.5          # nn.Embedding's N(0, 1)


def test_single_stream_has_no_modal_embedding():
    m = build_model(mm_config(64, [48], 4, 128, 1, 1), 131, "cpu", torch.float32)
    assert not any("modal_emb" in k for k in m.state_dict())


def test_buckets_tile_the_flat_buffer_with_new_parameters_last():
    m = build_model(mm_config(64, [48, 24, 16], 4, 128, 2, 2), 131, "cpu", torch.float32)
    ps = m._ps
    b = m.grad_buckets()
    assert b[0][0] == 0 and b[-1][1] == ps.total and all(b[i][1] == b[i + 1][0] for i in range(len(b) - 1))
    last = b[m.bucket_index("enc_layer", 0)]
    assert last == b[-1]
    names = ps.names
    u0 = names.index("video_encoder.unify.0.bias")
    new = ["video_encoder.unify.1.weight", "video_encoder.unify.1.bias", "video_encoder.unify.2.weight", "video_encoder.unify.2.bias",
           "video_encoder.modal_emb.modal_emb.weight"]
    assert names[u0 + 1:u0 + 1 + len(new)] == new
    for n in new:
        assert last[0] <= ps.offsets[n] < last[1], n
        p = dict(m.named_parameters())[n]
        assert p.data_ptr() == ps.flat.data_ptr() + 4 * ps.offsets[n]


def test_weight_file_and_training_state_round_trip(tmp_path):
    from vct_amd import checkpoint as ck
    mc = mm_config(64, [48, 24], 4, 128, 1, 1)
    p = mm_params(mc, 131, 9)
    a = build_model(mc, 131, "cpu", torch.float32, p)
    ck.save_weights(a, str(tmp_path / "w.pt"))
    b = build_model(mc, 131, "cpu", torch.float32)
    ck.load_weights(b, str(tmp_path / "w.pt"))
    for k in ("video_encoder.modal_emb.modal_emb.weight", "video_encoder.unify.1.weight", "video_encoder.unify.1.bias"):
        assert torch.equal(a.state_dict()[k], b.state_dict()[k]) and np.array_equal(b.state_dict()[k].numpy(), p[k])
    ck.save_training_state(str(tmp_path / "s.pt"), a, epoch=2)
    c = build_model(mc, 131, "cpu", torch.float32)
    info = ck.load_training_state(str(tmp_path / "s.pt"), c)
    assert info["epoch"] == 3
    assert torch.equal(c.state_dict()["video_encoder.modal_emb.modal_emb.weight"], a.state_dict()["video_encoder.modal_emb.modal_emb.weight"])
    assert c._ps.intact()


def test_frontend_entry_points_reject_bad_arguments():
    import __graft_entry__ as g
    g.build()
    from vct_amd import _lib
    lib = _lib.load()
    assert lib.vct_mm_frontend_fwd(None, None) == -1
    assert lib.vct_mm_frontend_bwd(None, None) == -1
    d = _lib.MmFrontendDesc()
    d.dtype, d.n, d.B, d.d, d.n_labels = 0, 2, 2, 64, 4
    d.T[0], d.T[1] = 3, 2
    assert lib.vct_mm_frontend_fwd(d, None) == -1          # null labels / inputs
    d.labels = 16
    assert lib.vct_mm_frontend_fwd(d, None) == -1          # null unify outputs
    d.dtype = 5
    assert lib.vct_mm_frontend_fwd(d, None) == -1          # bad dtype
    d.dtype, d.n = 0, 1
    assert lib.vct_mm_frontend_fwd(d, None) == -2          # one modality: the single-stream kernels' job
    d.n = _lib.MM_MAX_MODAL + 1
    assert lib.vct_mm_frontend_bwd(d, None) == -2
    d.n, d.n_labels = 2, 3
    assert lib.vct_mm_frontend_fwd(d, None) == -2          # label rows must be n or 2n
    d.n_labels, d.T[0] = 4, 0
    assert lib.vct_mm_frontend_bwd(d, None) == -2          # empty modality
    d.T[0], d.d = 3, 66
    assert lib.vct_mm_frontend_fwd(d, None) == -3          # width not a multiple of the vector
    d.d, d.T[0] = 64, 2000
    assert lib.vct_mm_frontend_fwd(d, None) == -2          # S > 1024
    d.T[0] = 3
    for i in range(2):
        d.u[i], d.du[i] = 4096 + 8, 4096                    # misaligned unify output
    d.temp, d.modal_w, d.x0 = 4096, 4096, 4096
    assert lib.vct_mm_frontend_fwd(d, None) == -3
    d.dx, d.d_modal = 4096 + 4, 4096
    assert lib.vct_mm_frontend_bwd(d, None) == -3


def test_stream_count_mismatch_and_limits_raise():
    """A model with two streams never quietly runs the one-stream path (unify.1 / modal_emb would get no gradient and be stepped with
    stale ones); more than 64 memory rows and a label table that does not match the modal embedding are errors, not wrong numbers."""
    mc = mm_config(64, [48, 24], 4, 128, 1, 1)
    m = build_model(mc, 131, "cpu", torch.float32, mm_params(mc, 131, 3))
    f = [torch.randn(2, 5, 48), torch.randn(2, 3, 24)]
    ids = torch.tensor([[101, 200, 102], [101, 300, 102]])
    with pytest.raises(ValueError):
        m.train_step_kernels(f[0], None, ids)             # a bare tensor
    with pytest.raises(ValueError):
        m.train_step_kernels(f[:1], None, ids)            # one stream short
    with pytest.raises(ValueError):
        m.greedy_decode_ids(f[0], None, max_len=4)
    with pytest.raises(ValueError):
        m(f[:1], None, ids)
    with pytest.raises(ValueError):
        m.train_step_kernels([torch.randn(2, 40, 48), torch.randn(2, 40, 24)], None, ids)   # S = 82 > 64 attention rows
    enc = m.video_encoder._engine()
    enc.cfg["modal_different"] = False                    # 2 labels against the 4 rows of modal_emb
    with pytest.raises(ValueError):
        enc.mm_rows((5, 3))
    enc.cfg["modal_different"] = True
    temp, labels = enc.mm_rows((5, 3))
    assert labels.tolist() == [2, 0, 0, 0, 0, 0, 3, 1, 1, 1] and temp.shape == (10, 64)
    assert float(temp[0].abs().sum()) == 0.0 and float(temp[6].abs().sum()) == 0.0
