"""Cross-attention maps on the GPU (csrc/vct_attn_weights.hip, caption_decoder.layer_type, decode return_attn):

  * the kernel against the fp64 numpy reference (tests/attnmap_ref.py) in bf16 and fp32: the fixture's shape, the decode use
    (Lq = 1, strided K batches, strided output row), ragged multi-tile shapes, the shape limits, causal + id padding, key_pad with a
    shift, a fully padded row (all zero, finite); row sums, bitwise run-to-run, and maps @ V == vct_attn_fwd's O at one head;
  * the model with `layer_type` against the reference's Vis decoder (tests/golden/attnmap_train.npz) in eval and train mode
    (dropout 0), on every executor, on the sample-stationary and the unfused stack;
  * decode: teacher-forced rows against the fixture, every step variant against the training forward of the same model, and the
    free-running session (graphs, replays, separate sessions).

Tolerances: kernel max-abs 1e-5 (fp32) / 1e-2 (bf16) x max(1, |want|max) as tests/test_encoder_variants_gpu.py; loss 1e-5 / 2e-3
relative, logits and maps 1e-4 / 2e-2 rel-Frobenius as tests/test_model_gpu.py (the model-against-fixture bf16 map bound is tightened
to 4 x the measured 1.23e-3)."""
import json

import numpy as np
import pytest
import torch

import vct_oracle as O
from attnmap_ref import attn_weights_ref
from helpers import GradTol, build_model, load_golden, model_config_of, rel

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _tol(dtype):
    return 1e-5 if dtype == F32 else 1e-2


def _close(got, want, tol):
    return np.abs(got - want).max() < tol * max(1.0, np.abs(want).max())


# ---- the kernel ----------------------------------------------------------------------------------------------------------------
def _qk(dtype, B, H, Lq, Lk, hd, seed, k_pad_rows=0):
    """q [B*Lq, D] and a K cache [B, Lk + k_pad_rows, D] (only the first Lk rows of a batch are keys) in `dtype`, and their exact
    fp64 values."""
    g = torch.Generator().manual_seed(seed)
    D = H * hd
    q = torch.randn(B * Lq, D, generator=g).to(dtype).to(DEV)
    kc = torch.randn(B, Lk + k_pad_rows, D, generator=g).to(dtype).to(DEV)
    qn = q.float().cpu().numpy().astype(np.float64).reshape(B, Lq, D)
    kn = kc.float().cpu().numpy().astype(np.float64)[:, :Lk]
    return q, kc, qn, kn


def _run(q, kc, B, H, Lq, Lk, w=None, **kw):
    from vct_amd import ops
    if w is None:
        w = torch.full((B, Lq, Lk), -7.0, dtype=F32, device=DEV)
    rows = kc.shape[1]
    ops.attn_weights(q, kc.view(B * rows, -1), w, B, H, Lq, Lk, kv_batch_stride=(rows * kc.shape[2] if rows != Lk else 0), **kw)
    return w


# the fixture's shape | the decode use | two query and key tiles, ragged tail, odd H | three tiles | the limits | both limits at once
# (fp32: the staged operands exceed 64 KB of LDS there)
SHAPES = [(3, 4, 6, 6, 16), (2, 8, 1, 13, 64), (2, 3, 19, 17, 32), (1, 2, 40, 40, 128), (2, 8, 64, 64, 64), (1, 1, 64, 64, 128)]


@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_vs_fp64(dtype, shape):
    B, H, Lq, Lk, hd = shape
    decode_use = Lq == 1
    q, kc, qn, kn = _qk(dtype, B, H, Lq, Lk, hd, seed=Lq * 100 + Lk, k_pad_rows=5 if decode_use else 0)
    want = attn_weights_ref(qn, kn, H)
    if decode_use:      # row 2 of layer 1 of a [B, layers 3, steps 4, Lk] buffer; everything else must stay untouched
        buf = torch.full((B, 3, 4, Lk), -7.0, dtype=F32, device=DEV)
        w = _run(q, kc, B, H, Lq, Lk, w=buf[:, 1, 2:3, :])
        keep = torch.ones_like(buf, dtype=torch.bool)
        keep[:, 1, 2] = False
        assert bool((buf[keep] == -7.0).all())
    else:
        w = _run(q, kc, B, H, Lq, Lk)
    got = w.cpu().numpy().astype(np.float64)
    err = np.abs(got - want).max()
    print(f"[attn-weights] {dtype} {shape}: max-abs {err:.3e}, row-sum dev {np.abs(got.sum(-1) - 1).max():.3e}")
    assert _close(got, want, _tol(dtype))
    assert np.abs(got.sum(-1) - 1.0).max() < _tol(dtype)
    w2 = _run(q, kc, B, H, Lq, Lk)
    assert torch.equal(w2, w.contiguous().view(B, Lq, Lk))          # fixed summation order: bitwise run to run


@pytest.mark.parametrize("dtype", [F32, BF])
def test_kernel_causal_and_id_padding(dtype):
    B, H, L, hd = 2, 3, 19, 32
    q, kc, qn, kn = _qk(dtype, B, H, L, L, hd, seed=7)
    ids = torch.randint(3, 90, (B, L + 2), generator=torch.Generator().manual_seed(5))
    ids[0, 15:] = 0
    ids[1, 17:] = 0
    want = attn_weights_ref(qn, kn, H, causal=True, key_pad=(ids[:, :L] == 0).numpy())
    w = _run(q, kc, B, H, L, L, causal=True, key_pad=("ids", ids.to(DEV), 0))
    got = w.cpu().numpy().astype(np.float64)
    assert _close(got, want, _tol(dtype))
    assert np.all(got[:, np.triu_indices(L, 1)[0], np.triu_indices(L, 1)[1]] == 0) and np.all(got[0, :, 15:] == 0)
    assert np.abs(got.sum(-1) - 1.0).max() < _tol(dtype)


@pytest.mark.parametrize("dtype", [F32, BF])
def test_kernel_key_pad_shift_and_fully_padded_row(dtype):
    B, H, L, hd = 3, 4, 6, 16
    q, kc, qn, kn = _qk(dtype, B, H, L, L, hd, seed=11)
    # shift 1: the mask covers keys 1.., key 0 is never padded -- a fully padded MASK row leaves all the weight on key 0
    m1 = torch.zeros(B, L - 1, dtype=torch.bool)
    m1[0, 3:] = True
    m1[1, :] = True
    got = _run(q, kc, B, H, L, L, key_pad=(m1.to(DEV), 1)).cpu().numpy().astype(np.float64)
    assert _close(got, attn_weights_ref(qn, kn, H, key_pad=m1.numpy(), shift=1), _tol(dtype))
    assert np.all(got[1, :, 1:] == 0) and np.abs(got[1, :, 0] - 1.0).max() < _tol(dtype)
    # shift 0: every key of sample 2 padded -> its rows are all zero and finite (the forward's inv = 0 rule), the others sum to 1
    m0 = torch.zeros(B, L, dtype=torch.bool)
    m0[0, 4:] = True
    m0[2, :] = True
    got = _run(q, kc, B, H, L, L, key_pad=m0.to(DEV)).cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all() and np.all(got[2] == 0)
    assert _close(got, attn_weights_ref(qn, kn, H, key_pad=m0.numpy()), _tol(dtype))
    assert np.abs(got[:2].sum(-1) - 1.0).max() < _tol(dtype)


@pytest.mark.parametrize("dtype", [F32, BF])
def test_one_head_map_times_v_is_the_forward_output(dtype):
    """H = 1, p_drop = 0: maps @ V must be vct_attn_fwd's O -- a map is the probability the forward used."""
    from vct_amd import ops
    B, L, Lk, hd = 2, 19, 17, 32
    q, kc, _qn, _kn = _qk(dtype, B, 1, L, Lk, hd, seed=3)
    v = torch.randn(B * Lk, hd, generator=torch.Generator().manual_seed(4)).to(dtype).to(DEV)
    o = torch.empty(B * L, hd, dtype=dtype, device=DEV)
    ops.attn_fwd(q, kc.view(B * Lk, hd), v, o, B, 1, L, Lk)
    w = _run(q, kc, B, 1, L, Lk)
    want = o.float().cpu().numpy().astype(np.float64).reshape(B, L, hd)
    got = w.cpu().numpy().astype(np.float64) @ v.float().cpu().numpy().astype(np.float64).reshape(B, Lk, hd)
    assert _close(got, want, _tol(dtype))


# ---- the model against the reference's Vis decoder -------------------------------------------------------------------------------
def _fixture():
    z = load_golden("attnmap_train.npz")
    mc = model_config_of(z)
    V = int(z["vocab"])
    p = O.init_params(O.cfg_from_model_config(mc, V), seed=int(z["param_seed"]))
    batch = tuple(torch.from_numpy(z[k]).to(DEV) for k in ("feats", "mask", "ids"))
    return z, mc, V, p, batch


# maps: the project's activation bounds are 1e-4 / 2e-2; the bf16 maps of this fixture measure 1.23e-3 (both layers, both modes: the
# near-uniform rows of a d = 64 model hide most of the bf16 rounding of q and K), so the bf16 bound is 4 x that, 5e-3
@pytest.mark.parametrize("dtype,tl,ta", [(F32, 1e-4, 1e-4), (BF, 2e-2, 5e-3)])
@pytest.mark.parametrize("mode", ["train", "eval"])
def test_model_maps_vs_reference(dtype, tl, ta, mode):
    z, mc, V, p, (feats, mask, ids) = _fixture()
    m = build_model(mc, V, DEV, dtype, p)
    m.train(mode == "train")           # dropout 0: both modes compute the fixture's forward
    loss, logits = m._forward_loss(feats, mask, ids, m.training, want_logits=True)
    assert abs(float(loss) - float(z["loss"])) < (1e-5 if dtype == F32 else 2e-3) * float(z["loss"])
    assert rel(logits[:, :V].float().reshape(z["act/logits"].shape), z["act/logits"]) < tl
    maps = m.cap_decoder.attn_weights
    assert isinstance(maps, list) and len(maps) == 2
    tol = GradTol(f"attn_maps_model_vs_reference({mode})", dtype, ta)
    for l, a in enumerate(maps):
        assert a.dtype == F32 and tuple(a.shape) == z[f"attn{l}"].shape
        tol.add(f"attn{l}", rel(a, z[f"attn{l}"]))
        assert float((a.sum(-1) - 1.0).abs().max()) < _tol(dtype)
    tol.report()
    # the reference-API path publishes the same maps
    before = [a.clone() for a in maps]
    m([feats], [mask], ids)
    assert all(torch.equal(a, b) for a, b in zip(m.cap_decoder.attn_weights, before))


def test_model_without_layer_type_has_no_maps():
    z, mc, V, p, (feats, mask, ids) = _fixture()
    mc = json.loads(json.dumps(mc))
    del mc["caption_decoder"]["layer_type"]
    m = build_model(mc, V, DEV, F32, p)
    m.train()
    m._forward_loss(feats, mask, ids, True)
    assert not hasattr(m.cap_decoder, "attn_weights")
    assert not any(isinstance(k, str) and k.endswith("ca.w") for k in m.cap_decoder._engine().cur.t)


def _trained_maps(executor, vis=True, steps=4, shapes=None):
    from test_executor_gpu import _batch
    from test_dist_gpu import MC, VOCAB
    from vct_amd.trainer import CaptionTrainer, FusedAdam
    mc = json.loads(json.dumps(MC))
    mc["dropout"] = 0.3
    if vis:
        mc["caption_decoder"]["layer_type"] = "vis"
    torch.manual_seed(7)
    m = build_model(mc, VOCAB, DEV, BF)
    m.train()
    m._seed.fill_(1234)
    tr = CaptionTrainer(m, FusedAdam(m, lr=1e-3), use_graph=executor == "graph", launch_list=executor == "list")
    losses, per_step = [], []
    for k in range(steps):
        kw = {} if shapes is None else dict(zip(("B", "T", "S"), shapes[k % len(shapes)]))
        losses.append(tr.step(*_batch(100 + k, **kw)).clone())
        if shapes is not None:
            per_step.append([a.clone() for a in m.cap_decoder.attn_weights])
    torch.cuda.synchronize()
    if shapes is not None:
        return per_step, torch.cat(losses), tr, m
    maps = [a.clone() for a in m.cap_decoder.attn_weights] if vis else None
    return maps, torch.cat(losses), tr, m


@pytest.mark.parametrize("executor", ["list", "graph"])
def test_recorded_executors_publish_each_shapes_own_maps(executor):
    """A ragged epoch: two (B, T, S) shapes alternate, so from the third step on every step is a REPLAY of one shape's recording
    while the engine's shared buffers last saw the other shape in Python.  After every step cap_decoder.attn_weights must be that
    step's maps: the step's shape, bitwise the eager step's."""
    shapes = [(6, 7, 9), (4, 5, 7)]
    want, l0, _, _ = _trained_maps("eager", steps=7, shapes=shapes)
    got, l1, tr, _ = _trained_maps(executor, steps=7, shapes=shapes)
    assert len(tr._lists if executor == "list" else tr._graphs) == 2
    assert torch.equal(l0, l1)
    for k, (w, g) in enumerate(zip(want, got)):
        B, T, S = shapes[k % 2]
        for a, b in zip(w, g):
            assert tuple(b.shape) == (B, S - 1, T + 1), (k, tuple(b.shape))
            assert torch.equal(a, b), k


def test_executors_give_bitwise_equal_maps():
    """Eager, recorded launch list and hipGraph (steps 2.. are replays): the maps of the last step, dropout on, are bitwise equal,
    and the recorded list of the model without `layer_type` is exactly `layers` launches shorter."""
    m0, l0, _, _ = _trained_maps("eager")
    m1, l1, tr_list, _ = _trained_maps("list")
    m2, l2, tr_graph, _ = _trained_maps("graph")
    assert tr_graph.use_graph and len(tr_graph._graphs) == 1 and len(tr_list._lists) == 1
    assert torch.equal(l0, l1) and torch.equal(l0, l2)
    for a, b, c in zip(m0, m1, m2):
        assert torch.equal(a, b) and torch.equal(a, c)
        assert float((a.sum(-1) - 1.0).abs().max()) < 1e-2          # probabilities BEFORE dropout: rows still sum to 1
    _, lp, tr_plain, mp = _trained_maps("list", vis=False)
    assert torch.equal(lp, l1)                                      # the maps change nothing the step computes
    (ll_vis, _a), = tr_list._lists.values()
    (ll_plain, _b), = tr_plain._lists.values()
    assert len(ll_vis) - len(ll_plain) == mp.cap_decoder.cfg["layers"] == 2


# ---- d = 512: the sample-stationary stack and every decode step variant ----------------------------------------------------------
def _mc512(vis=True):
    mc = json.loads(json.dumps(model_config_of(load_golden("cfgA_slices.npz"))))          # d = 512, 8 heads, features [512]
    mc["dropout"] = 0.0
    mc["video_encoder"].update(layer=1, feedforward=512)
    mc["caption_decoder"].update(layer=2, feedforward=512)
    if vis:
        mc["caption_decoder"]["layer_type"] = "vis"
    return mc


V512 = 131


def _model512(dtype=BF, vis=True):
    mc = _mc512(vis)
    return build_model(mc, V512, DEV, dtype, O.init_params(O.cfg_from_model_config(mc, V512), seed=23))


def test_sample_stationary_stack_maps_equal_the_unfused_schedule():
    from vct_amd import engine
    B, T, S = 2, 3, 5
    f, mk, ids = O.synthetic_batch(B, T, 512, S, V512, seed=4)
    feats, mask, idt = (torch.from_numpy(a).to(DEV) for a in (f, mk, ids))
    old = engine._StackBase.fuse_layers
    runs = {}
    try:
        for fused in (True, False):
            engine._StackBase.fuse_layers = fused
            m = _model512()
            m.train()
            assert m.cap_decoder._engine()._ss_ok(S - 1, T + 1, B) == fused
            m._forward_loss(feats, mask, idt, True)
            t = m.cap_decoder._engine().cur.t
            runs[fused] = ([a.clone() for a in m.cap_decoder.attn_weights],
                           [(t[f"L{l}.ca.q"].clone(), t[f"L{l}.ca.kv"][:, :512].clone()) for l in range(2)])
    finally:
        engine._StackBase.fuse_layers = old
    for l in range(2):
        (q1, k1), (q0, k0) = runs[True][1][l], runs[False][1][l]
        assert rel(q1, q0) < 2.5e-2 and rel(k1, k0) < 2.5e-2          # test_layer_ss_gpu's bound on the saved tensors
        e = rel(runs[True][0][l], runs[False][0][l])
        print(f"[attn-maps] layer {l}: stack vs unfused rel {e:.3e}; saved q/k bitwise equal: {torch.equal(q1, q0) and torch.equal(k1, k0)}")
        assert e < 2.5e-2
        if torch.equal(q1, q0) and torch.equal(k1, k0):
            assert torch.equal(runs[True][0][l], runs[False][0][l])


@pytest.mark.parametrize("dtype,ta", [(F32, 1e-4), (BF, 2e-2)])
def test_teacher_forced_rows_vs_reference(dtype, ta):
    from vct_amd import decode
    z, mc, V, p, (feats, mask, ids) = _fixture()
    m = build_model(mc, V, DEV, dtype, p)
    m.eval()
    steps = ids.shape[1] - 1
    out, maps = decode.teacher_forced_next_ids(m, feats, mask, ids, steps, return_attn=True)
    assert tuple(maps.shape) == (3, 2, steps, feats.shape[1] + 1) and maps.dtype == F32 and tuple(out.shape) == (3, steps)
    tol = GradTol("attn_maps_teacher_forced_vs_reference", dtype, ta)
    for b, fp in enumerate(z["first_pad"].tolist()):       # training masks padded keys in self-attention, decode has none
        assert fp >= 4
        for l in range(2):
            tol.add(f"attn{l}[{b}, :{fp}]", rel(maps[b, l, :fp], z[f"attn{l}"][b, :fp]))
    tol.report()


def test_greedy_ids_with_maps_are_the_reference_ids_fp32():
    """The fixture's greedy id matrix (reference loop on the same features, no mask, max_len 12) from the session that also
    returns maps."""
    z, mc, V, p, (feats, _mask, _ids) = _fixture()
    m = build_model(mc, V, DEV, F32, p)
    ys, maps = m.greedy_decode_ids([feats], None, max_len=12, return_attn=True)
    assert np.array_equal(ys.cpu().numpy(), z["greedy/ys"][:, :ys.shape[1]])
    assert tuple(maps.shape) == (3, 2, ys.shape[1] - 1, feats.shape[1] + 1)
    assert float((maps.sum(-1) - 1.0).abs().max()) < 1e-5


@pytest.mark.parametrize("variant", ["gemv", "fused", "generic"])
def test_decode_step_variants_vs_training_forward(variant):
    """Each step variant that can return maps, teacher-forced along pad-free captions, against the training forward of the same
    model (bf16, 2e-2 rel-Frobenius)."""
    from vct_amd import decode
    from vct_amd.engine import DecodeState, decode_step_variant
    B, T, max_len = (1 if variant == "gemv" else 2), 3, 6
    f, _mk, ids = O.synthetic_batch(B, T, 512, max_len, V512, seed=6)
    assert not (ids == 0).any()
    feats, idt = torch.from_numpy(f).to(DEV), torch.from_numpy(ids).to(DEV)
    m = _model512()
    m.eval()
    eng = m.cap_decoder._engine()
    m._forward_loss(feats, None, idt, False)
    want = [a.clone() for a in m.cap_decoder.attn_weights]            # [B, 5, Te]
    old = eng.fused_decode
    try:
        eng.fused_decode = variant != "generic"
        assert decode_step_variant(eng, DecodeState(eng, B, T + 1, max_len, return_attn=True)) == variant      # never 'block'
        _out, maps = decode.teacher_forced_next_ids(m, feats, None, idt, max_len - 1, return_attn=True)
    finally:
        eng.fused_decode = old
    tol = GradTol(f"attn_maps_decode_{variant}_vs_training_forward", BF, 2e-2)
    for l in range(2):
        tol.add(f"attn{l}", rel(maps[:, l], want[l]))
    tol.report()


@pytest.mark.parametrize("B", [1, 2])
def test_free_running_greedy_decode_with_maps(B):
    T, max_len = 3, 6
    feats = torch.from_numpy(O.synthetic_batch(B, T, 512, max_len, V512, seed=8)[0]).to(DEV)
    m = _model512(vis=False)               # return_attn is independent of layer_type
    eng = m.cap_decoder._engine()
    old = eng.block_decode
    try:
        eng.block_decode = False           # B = 1: the plain run on the step variant the map session takes (gemv), not the block step
        plain = m.greedy_decode_ids([feats], None, max_len=max_len)
        ys1, a1 = m.greedy_decode_ids([feats], None, max_len=max_len, return_attn=True)       # captures the graphs
        ys2, a2 = m.greedy_decode_ids([feats], None, max_len=max_len, return_attn=True)       # replays them
        ys3, a3 = m.greedy_decode_ids([feats], None, max_len=max_len, return_attn=True, use_graphs=False)
        again = m.greedy_decode_ids([feats], None, max_len=max_len)                           # its own session: untouched
    finally:
        eng.block_decode = old
    assert torch.equal(ys1, plain) and torch.equal(ys2, plain) and torch.equal(ys3, plain) and torch.equal(again, plain)
    assert tuple(a1.shape) == (B, 2, ys1.shape[1] - 1, T + 1) and a1.dtype == F32
    assert torch.equal(a1, a2) and torch.equal(a1, a3)
    assert float((a1.sum(-1) - 1.0).abs().max()) < 1e-2
    assert len(m._decode_sessions) == 2
    caps, a4 = m.greedy_decode([feats], None, max_len=max_len, return_attn=True)
    assert len(caps) == B and torch.equal(a4, a1)


def test_average_attention_on_device():
    from vct_amd.evaluate import average_attention
    z = load_golden("attnmap_train.npz")
    want = np.stack([z["attn0"], z["attn1"]], 1).mean(1)
    maps = torch.from_numpy(np.stack([z["attn0"], z["attn1"]], 1)).to(DEV)
    assert np.allclose(average_attention(maps).cpu().numpy(), want, atol=1e-7)
    assert np.allclose(average_attention(maps[2], 4).cpu().numpy(), want[2, :4], atol=1e-7)
