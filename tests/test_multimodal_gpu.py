"""Multi-modal video input (n >= 2 feature streams) on the GPU: the two front-end kernels against an fp64 restatement, parity
with the reference's MultiModalEncoder (tests/golden/mm_*.npz, tools/make_golden_multimodal.py), which paths the encoder and
decoder stacks take, bitwise determinism, and the loader / training / evaluation loops with two streams.

Tolerances as tests/test_model_gpu.py: fp32 loss 1e-5 rel, activations 1e-4, gradients 1e-3; bf16 logits 2e-2, loss 2e-3,
gradients 3e-2 (helpers.GradTol)."""
import json
import os

import numpy as np
import pytest
import torch

from helpers import GradTol, build_model, load_golden, model_config_of, rel
from mm_ref import mm_batch, mm_config, mm_params

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _inputs(z, n):
    return [_dev(z[f"feats{i}"]) for i in range(n)], [_dev(z[f"mask{i}"]) for i in range(n)], _dev(z["ids"])


def _model(z, dtype):
    mc = model_config_of(z)
    V = int(z["vocab"])
    return build_model(mc, V, DEV, dtype, mm_params(mc, V, int(z["param_seed"]))), mc, V


# ---- kernels ---------------------------------------------------------------------------------------------------------------
def _ref_frontend(us, masks, temp, modal, labels, B, Ts):
    d = us[0].shape[1]
    S = sum(t + 1 for t in Ts)
    x = np.zeros((B, S, d))
    kp = np.zeros((B, S), np.uint8)
    at = 0
    for i, t in enumerate(Ts):
        u = us[i].reshape(B, t, d)
        x[:, at] = u.mean(1)
        x[:, at + 1:at + 1 + t] = u
        if masks is not None:
            kp[:, at + 1:at + 1 + t] = masks[i]
        at += t + 1
    x += (temp + modal[labels])[None]
    return x, kp


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("Ts,B,diff", [((3, 2), 3, True), ((1, 1), 1, True), ((4, 1, 2), 2, False), ((5, 3, 2, 1), 4, True)])
def test_frontend_kernels_vs_fp64(dtype, Ts, B, diff):
    from vct_amd import ops
    torch.manual_seed(0)
    n, d = len(Ts), 64
    S = sum(t + 1 for t in Ts)
    nl = 2 * n if diff else n
    us = [torch.randn(B * t, d, device=DEV).to(dtype) for t in Ts]
    masks = [(torch.rand(B, t, device=DEV) < 0.4) for t in Ts]
    temp = torch.randn(S, d, device=DEV)
    modal = torch.randn(nl, d, device=DEV)
    labels, at = [], 0
    for i, t in enumerate(Ts):
        labels += [i + n if diff else i] + [i] * t
    lab = torch.tensor(labels, dtype=torch.int32, device=DEV)
    x0 = torch.full((B * S, d), float("nan"), device=DEV).to(dtype)
    kp = torch.full((B, S), 7, dtype=torch.uint8, device=DEV)
    ops.mm_frontend_fwd(us, [m.view(torch.uint8) for m in masks], temp, modal, lab, x0, kp, B, Ts)
    un = [u.double().cpu().numpy() for u in us]
    want, want_kp = _ref_frontend(un, [m.cpu().numpy() for m in masks], temp.double().cpu().numpy(), modal.double().cpu().numpy(),
                                  np.array(labels), B, Ts)
    tol = 1e-5 if dtype == torch.float32 else 1e-2
    assert np.abs(x0.double().cpu().numpy().reshape(B, S, d) - want).max() < tol * max(1.0, np.abs(want).max())
    assert np.array_equal(kp.cpu().numpy(), want_kp)
    # backward
    dx = torch.randn(B * S, d, device=DEV).to(dtype)
    dus = [torch.full((B * t, d), float("nan"), device=DEV).to(dtype) for t in Ts]
    dmod = torch.full((nl, d), float("nan"), device=DEV)
    ops.mm_frontend_bwd(dx, dus, dmod, lab, B, Ts)
    g = dx.double().cpu().numpy().reshape(B, S, d)
    at = 0
    for i, t in enumerate(Ts):
        want_du = g[:, at + 1:at + 1 + t] + g[:, at:at + 1] / t
        assert np.abs(dus[i].double().cpu().numpy().reshape(B, t, d) - want_du).max() < tol * max(1.0, np.abs(want_du).max()), i
        at += t + 1
    want_mod = np.zeros((nl, d))
    for s, l in enumerate(labels):
        want_mod[l] += g[:, s].sum(0)
    assert np.abs(dmod.double().cpu().numpy() - want_mod).max() < 1e-4 * max(1.0, np.abs(want_mod).max())
    dmod2 = torch.zeros_like(dmod)
    ops.mm_frontend_bwd(dx, dus, dmod2, lab, B, Ts)
    assert torch.equal(dmod, dmod2)                   # fixed reduction order: bitwise reproducible


# ---- reference parity --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,tl,tg", [(torch.float32, 1e-4, 1e-3), (torch.bfloat16, 2e-2, 3e-2)])
def test_two_streams_forward_backward_adam_vs_reference(dtype, tl, tg):
    z = load_golden("mm_train.npz")
    m, mc, V = _model(z, dtype)
    m.train()
    feats, masks, ids = _inputs(z, 2)
    loss, logits = m._forward_loss(feats, masks, ids, True, want_logits=True)
    lg = logits[:, :V].float().reshape(z["act/logits"].shape)
    assert rel(lg, z["act/logits"]) < tl
    assert abs(float(loss) - float(z["loss"])) < (1e-5 if dtype == torch.float32 else 2e-3) * float(z["loss"])
    enc_b = m.video_encoder._engine().cur
    assert rel(enc_b.t["x0"].float().view(z["act/mm_src"].shape), z["act/mm_src"]) < tl
    assert rel(enc_b.t["nf.y"].float().view(z["act/memory"].shape), z["act/memory"]) < tl
    # the module API: memory, the concatenated mask, the agg row
    mem, gmask, agg = m.video_encoder(feats, masks)
    assert rel(mem, z["act/memory"]) < tl and rel(agg, z["act/agg"]) < tl
    assert np.array_equal(gmask.cpu().numpy(), z["act/gmask"])
    opt = torch.optim.Adam(filter(lambda q: q.requires_grad, m.parameters()), lr=1e-4, betas=(0.9, 0.999))
    loss2 = m(feats, masks, ids)
    opt.zero_grad()
    loss2.backward()
    named = dict(m.named_parameters())
    tol = GradTol("mm_two_streams_vs_reference", dtype, tg)
    gk = [k[len("grad/"):] for k in z.files if k.startswith("grad/")]
    assert "video_encoder.modal_emb.modal_emb.weight" in gk and "video_encoder.unify.1.weight" in gk
    for k in gk:
        tol.add(k, rel(named[k].grad, z["grad/" + k]))
    tol.report()
    if dtype == torch.float32:
        p = {k: named[k].detach().cpu().numpy().astype(np.float64) for k in gk}
        opt.step()
        za = load_golden("mm_train_adam.npz")
        for k in gk:
            upd_ref = za["adam1/" + k].astype(np.float64) - p[k]
            upd = named[k].detach().cpu().numpy().astype(np.float64) - p[k]
            big = np.abs(z["grad/" + k]) > 1e-5
            assert np.abs(upd - upd_ref)[big].max(initial=0) < 5e-6, k


def test_three_streams_shared_modal_rows_vs_reference():
    z = load_golden("mm_train3.npz")
    m, mc, V = _model(z, torch.float32)
    assert tuple(m.video_encoder.modal_emb.modal_emb.weight.shape) == (3, 64)
    m.train()
    feats, masks, ids = _inputs(z, 3)
    loss = m(feats, masks, ids)
    assert abs(float(loss.detach()) - float(z["loss"])) < 1e-5 * float(z["loss"])
    assert rel(m.video_encoder._engine().cur.t["nf.y"].float().view(z["memory"].shape), z["memory"]) < 1e-4
    loss.backward()
    named = dict(m.named_parameters())
    for k in [k[len("grad/"):] for k in z.files if k.startswith("grad/")]:
        assert rel(named[k].grad, z["grad/" + k]) < 1e-3, k


@pytest.mark.parametrize("B", [1, 3])
def test_greedy_ids_exact_fp32(B):
    z = load_golden("mm_train.npz")
    zd = load_golden("mm_decode.npz")
    m, _mc, _V = _model(z, torch.float32)
    f = [_dev(zd[f"b{B}/feats0"]), _dev(zd[f"b{B}/feats1"])]
    want = zd[f"b{B}/ys"]
    for masks in (None, [torch.zeros(B, 5, dtype=torch.bool, device=DEV), torch.zeros(B, 3, dtype=torch.bool, device=DEV)]):
        ys = m.greedy_decode_ids(f, masks, max_len=12)
        assert np.array_equal(ys.cpu().numpy()[:, :want.shape[1]], want)
        ys_ref = m.greedy_decode_ids(f, masks, max_len=12, kv_cache=False)
        assert torch.equal(ys, ys_ref)
    # beam K = 1 is greedy
    b1 = m.beam_decode_ids(f, None, beam_size=1, max_len=12)
    g = m.greedy_decode_ids(f, None, max_len=12)
    for r in range(B):
        row = g[r].tolist()
        n = row.index(102) + 1 if 102 in row[1:] else len(row)
        assert b1[r].tolist()[:n] == row[:n]


class _Paths:
    """Which engines ran a sample-stationary stack (engine._StackBase._stack_ss) during the block."""

    def __enter__(self):
        from vct_amd import engine
        self.seen, self.orig = [], engine._StackBase._stack_ss
        seen, orig = self.seen, self.orig

        def spy(eng, *a, **k):
            seen.append(type(eng).__name__)
            return orig(eng, *a, **k)
        engine._StackBase._stack_ss = spy
        return self

    def __exit__(self, *exc):
        from vct_amd import engine
        engine._StackBase._stack_ss = self.orig


def test_cfgC_bf16_vs_reference_and_paths():
    """d 512, T = (12, 8): S = 22 -> the encoder runs sample-stationary, the decoder (22 > 16 memory rows) unfused."""
    z = load_golden("mm_cfgC_slices.npz")
    mc = model_config_of(z)
    V = int(z["vocab"])
    m = build_model(mc, V, DEV, torch.bfloat16, mm_params(mc, V, int(z["param_seed"])))
    m.train()
    f, k, ids = mm_batch(8, (12, 8), (512, 128), 20, V, seed=int(z["batch_seed"]),
                         valid=[[12, 10, 12, 9, 12, 12, 11, 12], [8, 8, 6, 8, 7, 8, 8, 5]])
    feats, masks, ids = [_dev(a) for a in f], [_dev(a) for a in k], _dev(ids)
    with _Paths() as pth:
        loss, logits = m._forward_loss(feats, masks, ids, True, want_logits=True)
    assert pth.seen == ["EncoderEngine"]
    assert abs(float(loss) - float(z["loss"])) < 2e-3 * float(z["loss"])
    lg = logits[:, :V].float().reshape(8, -1, V)
    assert rel(lg[:, :, :96], z["logits_head"]) < 2e-2
    mem = m.video_encoder._engine().cur.t["nf.y"].float().view(8, 22, 512)
    assert rel(mem[:, :, :64], z["memory_head"]) < 2e-2
    m.zero_grad()
    m(feats, masks, ids).backward()
    named = dict(m.named_parameters())
    tol = GradTol("mm_cfgC_bf16", torch.bfloat16, 3e-2)
    for name, norm in zip(json.loads(str(z["grad_names"])), z["grad_norms"]):
        g = named[name].grad.double()
        tol.add(name, abs(float(g.norm()) - float(norm)) / max(float(norm), 1e-30))
    tol.add("modal_emb", rel(named["video_encoder.modal_emb.modal_emb.weight"].grad, z["modal_emb_grad"]))
    tol.add("unify.1.head", rel(named["video_encoder.unify.1.weight"].grad[:64], z["unify1_grad_head"]))
    tol.report()


def _full_model(shapes, dtype=torch.bfloat16, seed=5):
    mc = mm_config(512, shapes, 8, 2048, 2, 2)
    return build_model(mc, 1000, DEV, dtype, mm_params(mc, 1000, seed))


def test_small_S_both_stacks_sample_stationary_matches_unfused():
    """T = (6, 4): S = 12 <= 16 memory rows -> both stacks sample-stationary; equal to the layer-by-layer schedule in bf16."""
    from vct_amd import engine
    m = _full_model([512, 128])
    m.train()
    f, k, ids = mm_batch(6, (6, 4), (512, 128), 9, 1000, seed=3, valid=[[6, 5, 6, 4, 6, 6], [4, 4, 2, 4, 3, 4]])
    feats, masks, ids = [_dev(a) for a in f], [_dev(a) for a in k], _dev(ids)
    with _Paths() as pth:
        l1 = m.train_step_kernels(feats, masks, ids).clone()
    assert sorted(pth.seen) == ["DecoderEngine", "EncoderEngine"]
    g1 = m.flat_grads.clone()
    old = engine._StackBase.fuse_layers
    engine._StackBase.fuse_layers = False
    try:
        with _Paths() as pth2:
            l2 = m.train_step_kernels(feats, masks, ids).clone()
        assert pth2.seen == []
    finally:
        engine._StackBase.fuse_layers = old
    assert abs(float(l1) - float(l2)) < 2e-3 * abs(float(l2))
    assert rel(g1, m.flat_grads) < 3e-2


def test_long_S_runs_the_encoder_layer_by_layer():
    """T = (20, 16): S = 38 > 32 rows -> layer by layer; the gradient still reaches both unify weights and the modal rows."""
    m = _full_model([512, 128])
    m.train()
    f, k, ids = mm_batch(4, (20, 16), (512, 128), 9, 1000, seed=4, valid=[[20, 18, 20, 11], [16, 9, 16, 16]])
    feats, masks, ids = [_dev(a) for a in f], [_dev(a) for a in k], _dev(ids)
    with _Paths() as pth:
        loss = m.train_step_kernels(feats, masks, ids)
    assert pth.seen == [] and torch.isfinite(loss).all()
    for n in ("video_encoder.unify.0.weight", "video_encoder.unify.1.weight", "video_encoder.modal_emb.modal_emb.weight"):
        assert float(m._ps.g[n].abs().sum()) > 0, n          # (train_step_kernels writes the flat gradient buffer)


# ---- determinism ---------------------------------------------------------------------------------------------------------------
def test_bitwise_determinism_and_executors():
    from vct_amd.trainer import CaptionTrainer, FusedAdam
    f, k, ids = mm_batch(8, (6, 4), (512, 128), 9, 1000, seed=6, valid=[[6] * 8, [4, 3, 4, 2, 4, 4, 1, 4]])
    feats, masks, ids = [_dev(a) for a in f], [_dev(a) for a in k], _dev(ids)
    m = _full_model([512, 128])
    m.train()
    l1 = m.train_step_kernels(feats, masks, ids).clone()
    g1 = m.flat_grads.clone()
    l2 = m.train_step_kernels(feats, masks, ids).clone()
    assert torch.equal(l1, l2) and torch.equal(g1, m.flat_grads)
    results = []
    for mode in ("eager", "list", "graph"):
        mm = _full_model([512, 128])
        mm.train()
        opt = FusedAdam(mm, lr=1e-4)
        tr = CaptionTrainer(mm, opt, use_graph=(mode == "graph"), launch_list=(mode == "list"))
        losses = [tr.step(feats, masks, ids).clone() for _ in range(3)]
        torch.cuda.synchronize()
        if mode == "graph":
            assert tr.use_graph            # capture of the two-stream step worked (no silent fall-back to eager)
        results.append((torch.cat(losses), mm.flat_params.clone()))
    for lo, pa in results[1:]:
        assert torch.equal(lo, results[0][0]) and torch.equal(pa, results[0][1])


# ---- loader / training / evaluation ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def two_stream_split(tmp_path_factory):
    d = tmp_path_factory.mktemp("mm_split")
    rng = np.random.default_rng(0)
    words = ["a", "man", "is", "playing", "guitar", "dog", "runs", "on", "grass", "woman", "cooks", "food"]
    lines = []
    for v in range(10):
        vid = f"video{v}"
        for i, (E, T) in enumerate(((16, 3 + v % 5), (8, 1 + (v * 3) % 4))):
            os.makedirs(d / f"m{i}", exist_ok=True)
            np.save(d / f"m{i}" / f"{vid}.npy", (rng.standard_normal((T, E)) + v % 3).astype(np.float32))
        for c in range(2):
            lines.append(f"{vid} " + " ".join(words[(v + c + j) % len(words)] for j in range(3 + (v + c) % 4)))
    (d / "ann.txt").write_text("\n".join(lines) + "\n")
    return d


def _mm_dataset(d, mode):
    from vct_amd import data
    return data.MSVD_Dataset([str(d / "m0"), str(d / "m1")], str(d / "ann.txt"), split_type="train", mode=mode)


def _toy_model(dtype=torch.float32, seed=3):
    from test_data_cpu import ToyTok
    mc = mm_config(64, [16, 8], 4, 128, 2, 2)
    torch.manual_seed(seed)
    m = build_model(mc, 2000, DEV, dtype)
    m.cap_preprocessor.tokenizer = ToyTok()
    return m


@pytest.mark.parametrize("mode", ["by_caption", "by_video"])
def test_device_loader_two_streams_equals_collate(two_stream_split, mode):
    from torch.utils.data import DataLoader
    from test_data_cpu import ToyPrep
    from vct_amd import data
    ds = _mm_dataset(two_stream_split, mode)
    dl = data.DeviceLoader(ds, 4, ToyPrep(), DEV, shuffle=False)
    host = DataLoader(ds, batch_size=4, collate_fn=data.collate_fn, shuffle=False)
    n = 0
    for (f, k, _caps, vids), (hf, hk, _hc, hv) in zip(dl, host):
        assert len(f) == len(k) == 2 and tuple(vids) == tuple(hv)
        for i in range(2):
            assert torch.equal(f[i].cpu(), hf[i]) and torch.equal(k[i].cpu(), hk[i])
        n += 1
    assert n == len(dl) == len(host)


def test_train_epoch_and_eval_two_streams(two_stream_split):
    from test_data_cpu import ToyPrep
    from vct_amd import data, evaluate
    from vct_amd.trainer import FusedAdam, train_epoch
    ds = _mm_dataset(two_stream_split, "by_caption")
    m = _toy_model(torch.bfloat16)
    opt = FusedAdam(m, lr=1e-3)
    dl = data.DeviceLoader(ds, 4, ToyPrep(), DEV, shuffle=True, seed=1)
    first = train_epoch(m, opt, dl)
    for e in range(1, 10):
        dl.set_epoch(e)
        last = train_epoch(m, opt, dl)
    assert np.isfinite(first) and last < 0.85 * first
    vds = _mm_dataset(two_stream_split, "by_video")
    vdl = data.DeviceLoader(vds, 4, ToyPrep(), DEV, shuffle=False)
    for beam in (None, 3):
        res = evaluate.eval_epoch(m, vdl, max_len=10, beam_size=beam)
        assert sorted(res) == sorted(f"video{v}" for v in range(10))
        assert all(isinstance(c, str) for c in res.values())
