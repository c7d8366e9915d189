"""The BASELINE.json configurations that earlier rounds only covered in reduced form:

  configs[1]  cfg-B at the full batch 256 against the numpy oracle (loss, logits element for element + log-sum-exp, every gradient
              tensor rel-Frobenius) + bitwise
              run-to-run determinism of the step;
  configs[3]  cfg-D: 6 + 6 layers, d_model 1024, head_dim 128, 32 frames, 40 tokens, V = 30522, batch 8 against slices recorded
              from the REAL reference (oracle/make_golden_cfgD.py), including the gradient-bucket cuts of a 6-layer stack;
  configs[4]  greedy decode of the d=512 model at batch 1 / 16 against the reference's ids (fp32, free-running, compared up to the
              first step whose top-2 margin is below the fp32 resolution) and at batch 128 against the oracle; bf16 teacher-forced.

Tolerances as in test_model_gpu.py (fp32: loss 1e-5 rel, gradients 1e-3; bf16: loss 1e-3, gradients 3e-2 = SURVEY 8(d); measured maximum over every tensor of every test 8.8e-3, profiles/r06_gpu_tests.txt)."""
import json

import numpy as np
import pytest
import torch

import vct_oracle as O
from helpers import GradTol, build_model, load_golden, model_config_of, rel

# bf16 tensors allowed above SURVEY 8(d)'s 3e-2 rel-Frobenius (they obey the test's own bound): filled in from the measured log
# (profiles/r06_gpu_tests.txt); None = record only
BF16_OVER_SURVEY = None

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _to_dev(*arrs):
    return [torch.from_numpy(a).to(DEV) for a in arrs]


@pytest.mark.parametrize("dtype,tl,tg", [(torch.float32, 1e-3, 1e-3), (torch.bfloat16, 2e-2, 3e-2)])
def test_cfgD_deep_model_vs_reference(dtype, tl, tg):
    z = load_golden("cfgD_slices.npz")
    mc, V = model_config_of(z), int(z["vocab"])
    cfg = O.cfg_from_model_config(mc, V)
    p = O.init_params(cfg, seed=int(z["param_seed"]))
    m = build_model(mc, V, DEV, dtype, p)
    assert sum(q.numel() for n, q in m.named_parameters() if not n.startswith("matching")) == int(z["n_params"])
    m.train()
    f, mk, ids = O.synthetic_batch(8, 32, 512, 40, V, seed=int(z["batch_seed"]), ragged=True)
    feats, mask, idt = _to_dev(f, mk, ids)
    loss, logits = m._forward_loss(feats, mask, idt, True, want_logits=True)
    lg = logits[:, :V].float().view(8, 39, V)
    assert rel(m.video_encoder._engine().cur.t["nf.y"].float().view(8, 33, 1024)[:, :, :64], z["memory_head"]) < tl
    assert rel(lg[:, :, :64], z["logits_head"]) < tl
    assert abs(float(loss) - float(z["loss"])) < (1e-5 if dtype == torch.float32 else 1e-3) * float(z["loss"])
    lse = torch.logsumexp(lg.double(), -1).cpu().numpy()
    assert np.abs(lse - z["logits_lse"]).max() < (1e-4 if dtype == torch.float32 else 3e-2)
    if dtype == torch.float32:
        valid = ids[:, 1:] != 0                                     # padded target rows carry no stable arg-max contract
        assert np.array_equal(lg.argmax(-1).cpu().numpy()[valid], z["logits_argmax"][valid])
    m._backward()
    names = json.loads(str(z["grad_names"]))
    tol = GradTol("cfgD_deep_model_vs_reference(norms)", dtype, tg)
    for i, k in enumerate(names):
        g = m._ps.g[k]
        n = float(g.double().norm())
        tol.add(k, abs(n - z["grad_norms"][i]) / max(float(z["grad_norms"][i]), 1e-30))
        head = np.resize(g.reshape(-1)[:32].cpu().numpy(), 32)
        assert np.abs(head - z["grad_heads"][i]).max() < tg * max(np.abs(z["grad_heads"][i]).max(), 1e-6) * 4 + 1e-8, k
    tol.report()


def test_cfgD_gradient_buckets_follow_the_backward_order():
    """A 6 + 6 layer stack: bucket i of grad_buckets() holds exactly the parameters whose gradients the backward schedule
    completes i-th (generator | decoder norm + layer 5 | layers 4..0 | token embedding | encoder norm + layer 5 | ... | layer 0 +
    unify), contiguous in the flat buffer, every cut a multiple of 64 elements (so it divides over 1/2/4/8 optimizer shards)."""
    z = load_golden("cfgD_slices.npz")
    mc, V = model_config_of(z), int(z["vocab"])
    m = build_model(mc, V, DEV, torch.bfloat16)
    ps, buckets = m._ps, m.grad_buckets()
    assert len(buckets) == 1 + 6 + 1 + 6
    assert buckets[0][0] == 0 and buckets[-1][1] == ps.total and all(b[1] == c[0] for b, c in zip(buckets, buckets[1:]))
    assert all(a % 64 == 0 and b % 64 == 0 for a, b in buckets)

    def names_in(i):
        a, b = buckets[i]
        return [n for n in ps.names if a <= ps.offsets[n] < b]
    assert names_in(0) == ["cap_decoder.generator.bias", "cap_decoder.generator.weight"] or set(names_in(0)) == {"cap_decoder.generator.bias", "cap_decoder.generator.weight"}
    for j, layer in enumerate(reversed(range(6))):
        got = names_in(1 + j)
        assert all(f"decoder.layers.{layer}." in n or (layer == 5 and "decoder.norm." in n) for n in got), (layer, got)
        assert m.bucket_index("dec_layer", layer) == 1 + j
    assert names_in(7) == ["cap_decoder.tgt_to_emb.weight"] and m.bucket_index("embedding") == 7
    for j, layer in enumerate(reversed(range(6))):
        got = [n for n in names_in(8 + j) if n.startswith("video_encoder.")]
        assert got and all(f"layers.{layer}." in n or (layer == 5 and "transformer_encoder.norm." in n) or (layer == 0 and "unify" in n)
                           for n in got), (layer, got)
        assert m.bucket_index("enc_layer", layer) == 8 + j
    # and the reference's own parameter order is a permutation of ours on the caption path
    ref_order = json.loads(str(z["param_order"]))
    assert sorted(ref_order) == sorted(n for n in ps.names if not n.startswith("matching"))


@pytest.mark.parametrize("dtype,tg", [(torch.float32, 1e-3), (torch.bfloat16, 3e-2)])
def test_cfgB_full_batch_256_vs_oracle(dtype, tg):
    mc = model_config_of(load_golden("cfgA_slices.npz"))           # the d=512 2+2 model of configs[0..2]
    V = 30522
    cfg = O.cfg_from_model_config(mc, V)
    p = O.init_params(cfg, seed=31)
    f, mk, ids = O.synthetic_batch(256, 12, 512, 20, V, seed=5)
    ref_loss, ref_grads, ref_logits = O.caption_loss_and_grads(p, cfg, f, mk, ids)
    rl = ref_logits.reshape(-1, V).astype(np.float64)
    ref_lse = np.log(np.exp(rl - rl.max(-1, keepdims=True)).sum(-1)) + rl.max(-1)
    m = build_model(mc, V, DEV, dtype, p)
    m.train()
    feats, mask, idt = _to_dev(f, mk, ids)
    loss, logits = m._forward_loss(feats, mask, idt, True, want_logits=True)
    if dtype == torch.bfloat16:
        # the benchmark configuration must be on the path bench.py times: sample-stationary stacks, one launch each -- a silent change
        # of the gate would otherwise leave every test green on the unfused fallback
        assert m.cap_decoder._engine()._ss_ok(19, 13, 256) and m.video_encoder._engine()._ss_ok(13, 0, 256)
        assert len(m._ps.packed) == 2
    lse = torch.logsumexp(logits[:, :V].double(), -1).cpu().numpy()
    assert abs(float(loss) - ref_loss) < (1e-5 if dtype == torch.float32 else 1e-3) * ref_loss
    assert np.abs(lse - ref_lse).max() < (1e-4 if dtype == torch.float32 else 3e-2)
    # the logits themselves, element for element, at the benchmark shape: rel-Frobenius <= 1e-3 (fp32) / 2e-2 (bf16)
    lerr = 0.0
    num = den = 0.0
    for r0 in range(0, rl.shape[0], 512):                          # in row chunks: 4864 x 30522 fp64 would be 1.2 GB per copy
        a = logits[r0:r0 + 512, :V].double().cpu().numpy()
        num += float(((a - rl[r0:r0 + 512]) ** 2).sum()); den += float((rl[r0:r0 + 512] ** 2).sum())
    lerr = (num / den) ** 0.5
    assert lerr < (1e-3 if dtype == torch.float32 else 2e-2), lerr
    del logits
    m._backward()
    tol = GradTol("cfgB_full_batch_256_vs_oracle", dtype, tg, allow_over_survey=BF16_OVER_SURVEY)
    for k, g in ref_grads.items():
        mine = m._ps.g[k].double().cpu().numpy()
        r = float(np.linalg.norm(g.astype(np.float64)))
        assert abs(float(np.linalg.norm(mine)) - r) < tg * r + 1e-9, (k, r)
        # full tensors, not only norms: a mis-routed or permuted gradient with the right norm must fail
        err = float(np.linalg.norm(mine - g.astype(np.float64).reshape(mine.shape))) / max(r, 1e-30)
        tol.add(k, err)
    tol.report()
    if dtype == torch.bfloat16:      # bitwise determinism of the full step at the benchmark batch (dropout 0.3 active)
        from vct_amd.trainer import CaptionTrainer, FusedAdam
        outs = []
        for _ in range(2):
            mm = build_model(dict(mc, dropout=0.3), V, DEV, dtype, p)
            mm.train(); mm._seed.fill_(99)
            tr = CaptionTrainer(mm, FusedAdam(mm, lr=1e-4), launch_list=True)
            losses = torch.cat([tr.step(feats, mask, idt).clone() for _ in range(3)])
            torch.cuda.synchronize()
            outs.append((losses, mm.flat_params.clone()))
            # the packed weight streams of the two stacks, maintained by the optimizer epilogues of the weight-gradient GEMMs at the
            # benchmark shape == a fresh pack of the shadow, bit for bit
            from vct_amd import ops
            for key, packed in mm._ps.packed.items():
                stream = packed.t
                fresh = ops.ss_pack([blk for part in packed.parts for blk in part.blocks], stream.clone())
                torch.cuda.synchronize()
                assert torch.equal(fresh.view(torch.int16), stream.view(torch.int16)), key
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def _compare_until_margin(ys, ref_ys, margins, thr):
    """Row by row: ids must agree up to (and including) the last step before the first top-2 margin below `thr`."""
    checked = 0
    for b in range(ref_ys.shape[0]):
        low = np.nonzero(margins[b] < thr)[0]
        upto = int(low[0]) + 1 if low.size else ref_ys.shape[1]      # column index: step t writes column t + 1
        upto = min(upto, ys.shape[1])
        assert np.array_equal(ys[b, :upto], ref_ys[b, :upto]), (b, ys[b, :upto], ref_ys[b, :upto])
        checked += upto
    return checked


def test_cfgB_greedy_decode_batch1_and_16_vs_reference():
    z = load_golden("cfgB_decode.npz")
    mc, V = model_config_of(z), int(z["vocab"])
    cfg = O.cfg_from_model_config(mc, V)
    p = O.init_params(cfg, seed=int(z["param_seed"]))
    m = build_model(mc, V, DEV, torch.float32, p)
    mb = build_model(mc, V, DEV, torch.bfloat16, p)
    for B in (1, 16):
        feats = torch.from_numpy(O.synthetic_batch(B, 12, 512, 20, V, seed=int(z[f"feats_seed_b{B}"]))[0]).to(DEV)
        ref_ys, margins = z[f"ys_b{B}"], z[f"margins_b{B}"]
        ys = m.greedy_decode_ids([feats], None, max_len=30).cpu().numpy()          # KV cache + captured per-token step
        n = _compare_until_margin(ys, ref_ys, margins, 5e-5)
        assert n > 0.9 * ref_ys.size
        ys_ref_alg = m.greedy_decode_ids([feats], None, max_len=30, kv_cache=False).cpu().numpy()
        _compare_until_margin(ys_ref_alg, ref_ys, margins, 5e-5)
        # bf16: teacher-forced next-token agreement wherever the reference's margin is resolvable in bf16
        memb = mb.video_encoder([feats], None)[0]
        ref = torch.from_numpy(ref_ys).to(DEV)
        agree = total = 0
        for t in range(1, 10):
            nxt = mb.cap_decoder.decode_word(memb, ref[:, :t], None).argmax(1).cpu().numpy()
            ok = margins[:, t - 1] > 0.15
            agree += int((nxt == ref_ys[:, t])[ok].sum()); total += int(ok.sum())
        assert agree == total


def test_cfgB_greedy_decode_batch128_vs_oracle():
    mc = model_config_of(load_golden("cfgB_decode.npz"))
    V = 30522
    cfg = O.cfg_from_model_config(mc, V)
    p = O.init_params(cfg, seed=778)
    f = O.synthetic_batch(128, 12, 512, 20, V, seed=21)[0]
    ref_ys, margins = O.greedy_decode_ids(p, cfg, f, None, max_len=10, return_margins=True)
    m = build_model(mc, V, DEV, torch.float32, p)
    ys = m.greedy_decode_ids([torch.from_numpy(f).to(DEV)], None, max_len=10).cpu().numpy()
    assert ys.shape == ref_ys.shape
    n = _compare_until_margin(ys, ref_ys, margins, 5e-5)
    assert n > 0.9 * ref_ys.size


@pytest.mark.parametrize("B,path", [(1, "block"), (1, "gemv"), (16, "skinny"), (128, "skinny"), (37, "skinny")])
def test_cfgB_bf16_kv_cache_step_teacher_forced(B, path, monkeypatch):
    """The bf16 token step that bench.py times -- batch 1: weight-streaming matrix-vector kernels (vct_decode_gemv / vct_decode_block),
    batch >= 2: skinny MFMA projections with LayerNorm prologues (vct_decode_linear) -- run through the KV cache along the reference's
    caption: the predicted next id must be the reference's wherever its top-2 logit margin is resolvable in bf16 (> 0.15),
    over >= 9 positions.  Batch 1 / 16: ids and margins recorded from the reference (cfgB_decode.npz); batch 128: the oracle.
    Batch 1 runs both of its kernels: one launch per layer block (vct_decode_block, the default) and one per stage (vct_decode_gemv)."""
    from vct_amd import decode, engine
    if path == "gemv":
        monkeypatch.setattr(engine.DecoderEngine, "block_decode", False)
    z = load_golden("cfgB_decode.npz")
    mc, V = model_config_of(z), int(z["vocab"])
    cfg = O.cfg_from_model_config(mc, V)
    steps = 10
    if B in (1, 16):
        p = O.init_params(cfg, seed=int(z["param_seed"]))
        f = O.synthetic_batch(B, 12, 512, 20, V, seed=int(z[f"feats_seed_b{B}"]))[0]
        ref_ys, margins = z[f"ys_b{B}"], z[f"margins_b{B}"]
    else:                                                          # 128, and 37: a ragged last row tile (37 = 2 * 16 + 5)
        p = O.init_params(cfg, seed=778)
        f = O.synthetic_batch(B, 12, 512, 20, V, seed=21)[0]
        ref_ys, margins = O.greedy_decode_ids(p, cfg, f, None, max_len=steps + 1, return_margins=True)
    assert ref_ys.shape[1] >= steps + 1
    mb = build_model(mc, V, DEV, torch.bfloat16, p)
    mb.eval()
    dec = mb.cap_decoder._engine()
    st = engine.DecodeState(dec, B, 13, steps + 1)
    if B == 1:                                                     # the path under test is the one that runs
        assert engine._decoder_block_decode_ok(dec, st) == (path == "block") and engine._decoder_small_decode_ok(dec, st)
    else:
        assert engine._decoder_fused_decode_ok(dec, st) and not engine._decoder_small_decode_ok(dec, st)
    feats = torch.from_numpy(f).to(DEV)
    ref = torch.from_numpy(np.ascontiguousarray(ref_ys[:, :steps + 1])).to(DEV)
    nxt, lgb = decode.teacher_forced_next_ids(mb, feats, None, ref, steps, return_logits=True)
    nxt = nxt.cpu().numpy()
    ok = margins[:, :steps] > 0.15
    assert ok.sum() >= 0.25 * ok.size and ok[:, :9].any(axis=0).sum() >= (9 if B > 1 else 4)
    assert np.array_equal(nxt[ok], ref_ys[:, 1:steps + 1][ok]), (nxt[ok] != ref_ys[:, 1:steps + 1][ok]).sum()
    if B <= 37:
        # every position, not only the clear-margin ones: the step's logits against the oracle's decode_word (bf16 tolerance)
        mem = O.mm_encoder_forward(p, cfg, f, None)[0]
        nb = min(B, 4)
        for t in range(1, steps + 1):
            want = O.decode_word(p, cfg, mem[:nb], ref_ys[:nb, :t])
            assert rel(lgb[:nb, t - 1], want) < 3e-2, (t, rel(lgb[:nb, t - 1], want))
    # the same step in fp32 (general kernels, exact-fp32 MFMA) agrees everywhere the margin is above fp32 resolution
    m32 = build_model(mc, V, DEV, torch.float32, p)
    m32.eval()
    nxt32, lg32 = decode.teacher_forced_next_ids(m32, feats, None, ref, steps, return_logits=True)
    ok32 = margins[:, :steps] > 5e-5
    assert np.array_equal(nxt32.cpu().numpy()[ok32], ref_ys[:, 1:steps + 1][ok32])
    if B <= 37:
        assert rel(lg32[:1, steps - 1], O.decode_word(p, cfg, mem[:1], ref_ys[:1, :steps])) < 1e-4


def test_shipped_width_fp32_batch1_decode_takes_the_batched_step():
    """d = 768 in fp32 is 3 sixteen-byte chunks per lane -- not a shape vct_decode_gemv has (1, 2, 4, 8): batch-1 decode (a
    ragged last eval batch, predict_video.py) must fall back to the batched step instead of raising, and still return the
    oracle's ids."""
    from vct_amd import engine
    mc = {"modal": ["clip"], "modal_shape": [512], "text_enc_type": "CLIP", "embed_dim": 768, "dropout": 0.3, "loss_beta": 0.5,
          "matching": None, "activation": "gelu",
          "video_encoder": {"layer": 1, "nhead": 8, "feedforward": 2048,
                            "mme": {"temporal": "encoding", "modal_different": True, "do_norm": False, "aggregation": "avg"}},
          "caption_decoder": {"layer": 3, "nhead": 8, "feedforward": 2048, "sce_loss_alpha": 0.5}, "pretrained_model": None}
    V = 1009
    cfg = O.cfg_from_model_config(mc, V)
    p = O.init_params(cfg, seed=5)
    f = O.synthetic_batch(1, 12, 512, 20, V, seed=3)[0]
    ref_ys, margins = O.greedy_decode_ids(p, cfg, f, None, max_len=8, return_margins=True)
    for dtype in (torch.float32, torch.bfloat16):
        m = build_model(mc, V, DEV, dtype, p)
        dec = m.cap_decoder._engine()
        st = engine.DecodeState(dec, 1, 13, 8)
        assert not engine._decoder_small_decode_ok(dec, st)        # (bf16: 768 = 1.5 x 512 is no whole chunk count either)
        ys = m.greedy_decode_ids([torch.from_numpy(f).to(DEV)], None, max_len=8).cpu().numpy()
        if dtype == torch.float32:
            _compare_until_margin(ys, ref_ys, margins, 5e-5)
        else:
            _compare_until_margin(ys, ref_ys, margins, 0.15)


def test_first_overlapped_step_leaves_exact_adam_moments(monkeypatch):
    """From zero moments the first step must leave m = (1 - b1) g and v = ((1 - b2) g) g of ITS OWN gradient, bitwise, for every
    parameter of the caption path -- at the bench batch, where Adam on the decoder / vocabulary part runs beside the encoder
    backward on the second stream.  Anything else means Adam read a gradient that was still being written, somebody else wrote the
    moment buffers, or the optimizer's arithmetic is not repeatable under co-scheduling (a v_sqrt / v_rcp + packed-fp32 variant of
    the kernel failed exactly this way: 16-lane groups of wrong first moments in generator.weight, a few per step)."""
    from vct_amd.trainer import CaptionTrainer, FusedAdam
    mc = model_config_of(load_golden("cfgA_slices.npz"))
    V = 30522
    p = O.init_params(O.cfg_from_model_config(mc, V), seed=31)
    f, mk, ids = O.synthetic_batch(256, 12, 512, 20, V, seed=5)
    feats, mask, idt = _to_dev(f, mk, ids)
    c1 = (torch.tensor(1.0) - torch.tensor(0.9)).to(DEV)
    c2 = (torch.tensor(1.0) - torch.tensor(0.999)).to(DEV)
    monkeypatch.setattr(FusedAdam, "keep_grads", True)      # the optimizer epilogue of the weight-gradient GEMMs also stores the gradient it consumed
    for drop, fuse in ((0.3, True), (0.0, True), (0.0, False)):
        mm = build_model(dict(mc, dropout=drop), V, DEV, torch.bfloat16, p)
        mm.train(); mm._seed.fill_(99)
        opt = FusedAdam(mm, lr=1e-4)
        tr = CaptionTrainer(mm, opt, launch_list=True)
        tr.fuse_adam = fuse
        tr.step(feats, mask, idt)
        torch.cuda.synchronize()
        e = mm.caption_param_end
        g = mm.flat_grads[:e]
        assert torch.equal(opt.exp_avg[:e], g * c1)
        assert torch.equal(opt.exp_avg_sq[:e], (g * c2) * g)


def test_batch1_decode_with_wide_feedforward_falls_back():
    """d = 512 / 8 heads but ff = 4096: ff / 64 = 64 partial vectors exceed what the block kernels' consumers sum (32), so the
    support predicate must say no and batch-1 decode must take the gemv / batched step -- same ids as the fp32 oracle path would
    give teacher-forced is covered elsewhere; here: the call succeeds and equals the small-batch (non-block) step's ids."""
    from vct_amd import _lib as L, engine
    assert L.load().vct_decode_block_supported(L.BF16, 512, 8, 2048, 13) == 1
    assert L.load().vct_decode_block_supported(L.BF16, 512, 8, 4096, 13) == 0
    mc = model_config_of(load_golden("cfgA_slices.npz"))
    mc = dict(mc); mc["caption_decoder"] = dict(mc["caption_decoder"], feedforward=4096, layer=1)
    mc["video_encoder"] = dict(mc["video_encoder"], layer=1)
    torch.manual_seed(3)
    m = build_model(mc, 997, DEV, torch.bfloat16)
    m.eval()
    feats = torch.randn(1, 12, 512, generator=torch.Generator().manual_seed(2)).to(DEV)
    ys = m.greedy_decode_ids([feats], None, max_len=10)
    st = next(iter(m.__dict__["_decode_sessions"].values()))
    assert not engine._decoder_block_decode_ok(m.cap_decoder._engine(), st)
    old = engine.DecoderEngine.block_decode
    try:
        engine.DecoderEngine.block_decode = False
        m2 = build_model(mc, 997, DEV, torch.bfloat16)
        m2.load_state_dict(m.state_dict()); m2.eval()
        ys2 = m2.greedy_decode_ids([feats], None, max_len=10)
    finally:
        engine.DecoderEngine.block_decode = old
    assert torch.equal(ys, ys2) and ys.shape[1] >= 2


@pytest.mark.parametrize("path", ["block", "gemv"])
def test_batch1_decode_at_the_key_count_limit(path, monkeypatch):
    """Both batch-1 steps at the limit their predicates admit: 63 frames (64 memory rows) and a 64-position session, teacher-forced
    along random ids through all 63 positions (self-attention over 1 .. 63 keys, cross-attention over 64).  Every position's
    logits against the oracle's decode_word under the bf16 bound of test_cfgB_bf16_kv_cache_step_teacher_forced; no margin
    filter, nothing left out."""
    from vct_amd import decode, engine
    if path == "gemv":
        monkeypatch.setattr(engine.DecoderEngine, "block_decode", False)
    mc = {"modal": ["clip"], "modal_shape": [512], "text_enc_type": "CLIP", "embed_dim": 512, "dropout": 0.3, "loss_beta": 0.5,
          "matching": None, "activation": "gelu",
          "video_encoder": {"layer": 1, "nhead": 8, "feedforward": 2048,
                            "mme": {"temporal": "encoding", "modal_different": True, "do_norm": False, "aggregation": "avg"}},
          "caption_decoder": {"layer": 2, "nhead": 8, "feedforward": 2048, "sce_loss_alpha": 0.5}, "pretrained_model": None}
    V, T, steps = 1009, 63, 63
    cfg = O.cfg_from_model_config(mc, V)
    p = O.init_params(cfg, seed=17)
    f = O.synthetic_batch(1, T, 512, 20, V, seed=9)[0]
    ids = np.random.default_rng(4).integers(1, V, (1, steps + 1)).astype(np.int64)
    m = build_model(mc, V, DEV, torch.bfloat16, p)
    m.eval()
    dec = m.cap_decoder._engine()
    st = engine.DecodeState(dec, 1, T + 1, steps + 1)
    assert (st.Te, st.Lmax) == (64, 64)
    assert engine._decoder_block_decode_ok(dec, st) == (path == "block") and engine._decoder_small_decode_ok(dec, st)
    assert engine.decode_step_variant(dec, st) == path
    feats = torch.from_numpy(f).to(DEV)
    assert decode.memory_len(feats) == T + 1
    _, lg = decode.teacher_forced_next_ids(m, feats, None, torch.from_numpy(ids).to(DEV), steps, return_logits=True)
    assert lg.shape == (1, steps, V) and bool(torch.isfinite(lg).all())
    mem = O.mm_encoder_forward(p, cfg, f, None)[0]
    assert mem.shape[1] == T + 1
    errs = [rel(lg[:, t - 1], O.decode_word(p, cfg, mem, ids[:, :t])) for t in range(1, steps + 1)]
    print(f"[key-count limit] {path}: worst logit error {max(errs):.3e} at position {int(np.argmax(errs)) + 1}")
    assert max(errs) < 3e-2, (int(np.argmax(errs)) + 1, max(errs))
