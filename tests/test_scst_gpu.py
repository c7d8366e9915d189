"""Self-critical sequence training on the GPU: vct_wce_loss and vct_group_sum against the float64 restatement (tests/scst_ref.py),
bitwise equality of the weighted loss at unit weights with vct_sce_loss(alpha = 1), the model-level step against the numpy oracle
with the features repeated N times (which pins the memory fan-out and the group sum), its reduction to the caption step, the
forward-only scoring and CaptionTrainer.scst_step.

Tolerances are the project's own for this arithmetic: the loss kernel's from test_kernels_gpu.test_sce_loss (loss 2e-5 relative,
dlogits relative Frobenius 2e-5 fp32 / 6e-3 bf16), log-probabilities as test_sample_gpu (rtol 1e-5, atol 1e-6), the model's from
test_model_gpu.test_tiny_forward_backward_adam_vs_reference (fp32: loss 1e-5, gradients 1e-3; bf16: loss 2e-3, gradients 3e-2)."""
import numpy as np
import pytest
import torch

import scst_ref as R
import vct_oracle as O
from helpers import GradTol, build_model, golden_params, load_golden, model_config_of, rel
from mm_ref import mm_params

pytestmark = pytest.mark.gpu
DEV = "cuda"
CANARY = 12345.0


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from vct_amd import ops as _ops
    return _ops


def rnd(*shape, dtype=torch.float32, scale=1.0, seed=0):       # test_kernels_gpu's generator
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(DEV)


def _guarded(rows, cols, dtype, fill=CANARY):
    """A [rows, cols] view with one canary row in front and one behind."""
    full = torch.full((rows + 2, cols), fill, dtype=dtype, device=DEV)
    return full, full[1:rows + 1]


def _guards_intact(full, fill=CANARY):
    return bool((full[0] == fill).all()) and bool((full[-1] == fill).all())


# ---- 1. vct_wce_loss against fp64 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("V", [7, 257, 30522])
def test_wce_loss_vs_fp64(ops, dtype, V):
    B, S, PAD = 3, 4, 3
    N = B * S
    Vp = (V + 31) // 32 * 32
    x = rnd(N, V, dtype=dtype, scale=9.0 if V < 1000 else 2.0, seed=70)
    g = torch.Generator().manual_seed(4)
    ids = torch.randint(4, V, (B, S + 1), generator=g)
    ids[0, 1], ids[0, 2] = 0, V - 1                 # the first and the last column as labels
    ids[1, 3:] = PAD                                # a pad tail
    ids[2, :] = PAD                                 # an all-pad sequence
    ids = ids.to(DEV)
    labels = ids[:, 1:]                             # the token-shift view: batch stride S + 1
    lab = labels.cpu().numpy()
    tol_d = 2e-5 if dtype == torch.float32 else 6e-3
    for wv in ([1000.0, -2.5, 0.0], [0.0, 1000.0, -2.5]):
        ref_loss, ref_d, ref_tok = R.wce_loss(x.double().cpu().numpy(), lab, wv, PAD)
        wfull = torch.full((B + 2,), CANARY, device=DEV)
        wfull[1:B + 1] = torch.tensor(wv)
        w = wfull[1:B + 1]

        def run(mode):
            lg_full, lg = _guarded(N, Vp, dtype)
            lg.fill_(float("nan"))                  # columns V.. are not logits: whatever they hold must not reach a result
            lg[:, :V] = x
            loss_full = torch.full((3,), CANARY, device=DEV)
            tok_full = torch.full((N + 2,), CANARY, device=DEV)
            ws_full = torch.full((2 * N + 2 + 2,), CANARY, device=DEV)
            if mode == "inplace":
                d_full, dl = lg_full, lg
            elif mode == "wide":
                d_full, dl = _guarded(N, Vp + 64, dtype)
            else:
                d_full, dl = None, None
            ops.wce_loss(lg, V, labels, S, PAD, w, loss_full[1:2], dl, ws_full[1:-1], tok_logp=tok_full[1:-1])
            torch.cuda.synchronize()
            assert loss_full[0] == CANARY and loss_full[2] == CANARY and tok_full[0] == CANARY and tok_full[-1] == CANARY
            assert ws_full[0] == CANARY and ws_full[-1] == CANARY and _guards_intact(lg_full)
            assert wfull[0] == CANARY and wfull[-1] == CANARY and torch.equal(w.cpu(), torch.tensor(wv))
            if d_full is not None:
                assert _guards_intact(d_full)
            if mode != "inplace":                   # the logits are read-only unless the gradient aliases them
                assert torch.equal(lg[:, :V], x) and bool(torch.isnan(lg[:, V:]).all())
            return loss_full[1:2].clone(), tok_full[1:-1].clone(), (None if dl is None else dl.clone())

        outs = {}
        for mode in ("inplace", "wide", "forward"):
            loss, tok, dl = outs[mode] = run(mode)
            err_l = abs(float(loss) - ref_loss) / abs(ref_loss)
            print(f"[wce] V={V} {dtype} w={wv} {mode}: loss rel err {err_l:.3g}"
                  + ("" if dl is None else f", dlogits rel {rel(dl[:, :V], ref_d):.3g}")
                  + f", tok_logp max abs err {np.abs(tok.cpu().numpy() - ref_tok).max():.3g}")
            assert err_l < 2e-5
            np.testing.assert_allclose(tok.cpu().numpy(), ref_tok, rtol=1e-5, atol=1e-6)
            pad_rows = torch.from_numpy(lab.reshape(-1) == PAD).to(DEV)
            assert bool((tok[pad_rows] == 0).all())
            if dl is not None:
                assert rel(dl[:, :V], ref_d) < tol_d
                assert bool((dl[pad_rows] == 0).all()) and bool((dl[:, V:] == 0).all())          # exact zeros
                z0 = torch.tensor([w_ == 0.0 for w_ in wv]).repeat_interleave(S).to(DEV)
                assert bool((dl[z0] == 0).all())                                                   # a zero advantage: no gradient
        # the three forms agree bit for bit, and a second call repeats the first
        assert torch.equal(outs["inplace"][0], outs["wide"][0]) and torch.equal(outs["inplace"][0], outs["forward"][0])
        assert torch.equal(outs["inplace"][1], outs["forward"][1])
        assert torch.equal(outs["inplace"][2][:, :V], outs["wide"][2][:, :V])
        again = run("wide")
        assert torch.equal(again[0], outs["wide"][0]) and torch.equal(again[1], outs["wide"][1]) and torch.equal(again[2], outs["wide"][2])


# ---- 2. unit weights are vct_sce_loss(alpha = 1), bit for bit ----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("V", [257, 30522])
def test_wce_loss_unit_weights_bitwise_equal_sce_alpha_1(ops, dtype, V):
    B, S = 6, 5
    N = B * S
    Vp = (V + 31) // 32 * 32
    lg = torch.zeros(N, Vp, dtype=dtype, device=DEV)
    lg[:, :V] = rnd(N, V, dtype=dtype, scale=9.0 if V < 1000 else 2.0, seed=70)
    g = torch.Generator().manual_seed(4)
    ids = torch.randint(1, V, (B, S + 1), generator=g).to(DEV)
    ids[1, 3:] = 0
    labels = ids[:, 1:]
    loss0, dl0, ws = torch.empty(1, device=DEV), torch.empty_like(lg), torch.empty(2 * N + 2, device=DEV)
    ops.sce_loss(lg, V, labels, S, 0, 1.0, loss0, dl0, ws)
    for w in (None, torch.ones(B, device=DEV)):
        loss1, dl1, ws1 = torch.full((1,), -1.0, device=DEV), torch.full_like(lg, 7.0), torch.empty(2 * N + 2, device=DEV)
        ops.wce_loss(lg, V, labels, S, 0, w, loss1, dl1, ws1)
        assert torch.equal(loss0, loss1)
        assert torch.equal(dl0.view(torch.int16 if dtype == torch.bfloat16 else torch.int32),
                           dl1.view(torch.int16 if dtype == torch.bfloat16 else torch.int32))          # the bits, not the values
    # ... in place as well (the gradient overwrites the logits)
    lg2 = lg.clone()
    loss2 = torch.empty(1, device=DEV)
    ops.wce_loss(lg2, V, labels, S, 0, None, loss2, lg2, ws)
    assert torch.equal(loss0, loss2) and torch.equal(dl0, lg2)


# ---- 3. vct_group_sum ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("d", [8, 64, 512])
@pytest.mark.parametrize("G", [1, 3, 5])
def test_group_sum_vs_fp64(ops, dtype, G, d):
    B, Rr = 2, 5
    x = rnd(B * G * Rr, d, dtype=dtype, scale=3.0, seed=90 + G)
    x[0, 0] = -0.0
    full, out = _guarded(B * Rr, d, dtype)
    ops.group_sum(x, out, B, G, Rr)
    torch.cuda.synchronize()
    assert _guards_intact(full)
    xd = x.double().cpu().numpy()
    want = R.group_sum(xd, B, G, Rr)
    got = out.double().cpu().numpy()
    mag = R.group_sum(np.abs(xd), B, G, Rr)
    if dtype == torch.float32:
        bound = G * 2.0 ** -24 * mag                              # G - 1 fp32 additions in ascending order
    else:
        bound = 2.0 ** -8 * np.abs(want) + G * 2.0 ** -24 * mag   # one rounding into bf16 behind the fp32 sum
    assert (np.abs(got - want) <= bound).all(), float((np.abs(got - want) - bound).max())
    if G == 1:
        it = torch.int16 if dtype == torch.bfloat16 else torch.int32
        assert torch.equal(out.view(it), x.view(it))             # a bitwise copy (-0 stays -0)
    full2, out2 = _guarded(B * Rr, d, dtype)
    ops.group_sum(x, out2, B, G, Rr)
    assert torch.equal(out, out2)


# ---- 4. the model-level step against the oracle with the features repeated N times ------------------------------------------------------
def _scst_ids(rows, L, V, seed):
    """Fixed id rows with ragged ends: start 101, body, end 102, pads (0) behind."""
    rng = np.random.default_rng(seed)
    ids = np.zeros((rows, L), np.int64)
    ids[:, 0] = 101
    for r in range(rows):
        n = 2 + (r * 2) % (L - 2)                                 # body + end token: 2 .. L - 1 tokens
        ids[r, 1:n] = rng.integers(103, V, n - 1)
        ids[r, n] = 102
    ids[0, 1:] = rng.integers(103, V, L - 1)                      # one row that never ends
    return ids


ADV = np.array([1.5, -0.5, 0.75, -1.0, 2.0, 0.25], np.float32)   # B = 2 videos x N = 3 samples, mixed sign


def _tiny(name="tiny_train.npz"):
    z = load_golden(name)
    mc = model_config_of(z)
    V = int(z["vocab"])
    cfg = O.cfg_from_model_config(mc, V)
    return z, mc, V, cfg, golden_params(z, cfg)


def _two_streams():
    z = load_golden("mm_train.npz")
    mc = model_config_of(z)
    V = int(z["vocab"])
    cfg = O.cfg_from_model_config(mc, V)
    p = mm_params(mc, V, int(z["param_seed"]))
    p[O.ENC + "temp_emb.pe"] = O.encoder_pos_table(512, cfg["d"])
    p[O.DEC + "positional_encoding.pos_embedding"] = O.decoder_pos_table(5000, cfg["d"])
    return z, mc, V, cfg, p


_REF = {}


def _reference(streams):
    """(model config, V, parameters, features, masks, ids, loss, gradients, tok_logp) -- computed once per stream count, shared."""
    if streams not in _REF:
        if streams == 1:
            z, mc, V, cfg, p = _tiny()
            feats, masks = [z["feats"][:2]], [z["mask"][:2]]
        else:
            z, mc, V, cfg, p = _two_streams()
            feats, masks = [z["feats0"][:2], z["feats1"][:2]], [z["mask0"][:2], z["mask1"][:2]]
        ids = _scst_ids(6, 7, V, seed=11)
        loss, grads, _mem, tok = R.scst_loss_and_grads(O, p, cfg, [np.repeat(f, 3, 0) for f in feats], [np.repeat(k, 3, 0) for k in masks],
                                                       ids, ADV)
        _REF[streams] = (mc, V, p, feats, masks, ids, loss, grads, tok)
    return _REF[streams]


@pytest.mark.parametrize("dtype,tl,tg", [(torch.float32, 1e-5, 1e-3), (torch.bfloat16, 2e-3, 3e-2)])
@pytest.mark.parametrize("streams", [1, 2])
def test_train_step_kernels_scst_vs_oracle(ops, streams, dtype, tl, tg):
    mc, V, p, feats, masks, ids, ref_loss, ref_grads, _ = _reference(streams)
    m = build_model(mc, V, DEV, dtype, p)
    m.train()                                                     # dropout is 0 in these configs
    f = [torch.from_numpy(a).to(DEV) for a in feats]
    k = [torch.from_numpy(a).to(DEV) for a in masks]
    if streams == 1:
        f, k = f[0], k[0]
    loss = m.train_step_kernels_scst(f, k, torch.from_numpy(ids).to(DEV), torch.from_numpy(ADV).to(DEV), num_samples=3)
    print(f"[scst] streams={streams} {dtype}: loss {float(loss):.7g} ref {ref_loss:.7g}")
    assert abs(float(loss) - ref_loss) < tl * abs(ref_loss)
    tol = GradTol(f"train_step_kernels_scst_vs_oracle_{streams}", dtype, tg)
    assert len(ref_grads) == len([n for n in m._ps.names if not n.startswith("matching.")])
    for name, g in ref_grads.items():
        tol.add(name, rel(m._ps.g[name], g))
    tol.report()
    assert m.grads_valid
    assert float(m._ps.g["cap_decoder.tgt_to_emb.weight"][0].abs().sum()) == 0.0
    # gradients are written, not accumulated: a second call leaves the same bits
    g1, l1 = m.flat_grads.clone(), loss.clone()
    l2 = m.train_step_kernels_scst(f, k, torch.from_numpy(ids).to(DEV), torch.from_numpy(ADV).to(DEV), num_samples=3)
    assert torch.equal(l1, l2) and torch.equal(g1, m.flat_grads)


# ---- 5. N = 1 with unit weights is the caption step -------------------------------------------------------------------------------------
def test_scst_reduces_to_the_caption_step(ops):
    z = load_golden("tiny_train_ce_relu.npz")                     # sce_loss_alpha = 1
    mc = model_config_of(z)
    V = int(z["vocab"])
    m = build_model(mc, V, DEV, torch.float32, O.init_params(O.cfg_from_model_config(mc, V), seed=12))
    m.train()
    feats, mask, ids = (torch.from_numpy(z[k]).to(DEV) for k in ("feats", "mask", "ids"))
    l0 = m.train_step_kernels(feats, mask, ids).clone()
    g0 = m.flat_grads.clone()
    named0 = {n: m._ps.g[n].clone() for n in m._ps.names if not n.startswith("matching.")}
    calls = []
    orig_sum, orig_wce = ops.group_sum, ops.wce_loss
    ops.group_sum = lambda *a, **kw: calls.append("sum") or orig_sum(*a, **kw)
    ops.wce_loss = lambda *a, **kw: calls.append("wce") or orig_wce(*a, **kw)
    try:
        l1 = m.train_step_kernels_scst(feats, mask, ids, torch.ones(ids.shape[0], device=DEV), num_samples=1)
    finally:
        ops.group_sum, ops.wce_loss = orig_sum, orig_wce
    assert calls == ["wce"]                                       # N = 1: no group sum (and no fan-out buffer)
    assert "scst.mem" not in m.cap_decoder._engine().cur.t
    assert torch.equal(l0, l1) and torch.equal(g0, m.flat_grads)
    # ... and every gradient is WRITTEN by the step (the alignment gaps between the parameters and matching.* are nobody's)
    m.flat_grads.fill_(3.0)
    l2 = m.train_step_kernels_scst(feats, mask, ids, torch.ones(ids.shape[0], device=DEV), num_samples=1)
    assert torch.equal(l0, l2)
    for n, g in named0.items():
        assert torch.equal(g, m._ps.g[n]), n


# ---- 6. score_captions ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_score_captions(ops, dtype):
    mc, V, p, feats, masks, ids_np, _, _, ref_tok = _reference(1)
    m = build_model(mc, V, DEV, dtype, p)
    m.train()                                                     # scoring runs with dropout off whatever the mode
    f, k = torch.from_numpy(feats[0]).to(DEV), torch.from_numpy(masks[0]).to(DEV)
    ids = torch.from_numpy(ids_np).to(DEV)
    m.flat_grads.fill_(5.0)
    before = m.flat_grads.clone()
    # N = 1 on the first two rows: the same forward as _forward_loss, whose logits give the reference
    ids2 = ids[[0, 3]].contiguous()
    seq, tok = m.score_captions([f], [k], ids2)
    _, logits = m._forward_loss(f, k, ids2, False, want_logits=True)
    lp = torch.log_softmax(logits[:, :V].double(), -1).view(2, ids2.shape[1] - 1, V)
    want = lp.gather(2, ids2[:, 1:, None]).squeeze(2)
    want = torch.where(ids2[:, 1:] == 0, torch.zeros_like(want), want)
    assert tok.shape == (2, ids2.shape[1] - 1) and tok.dtype == torch.float32 and seq.shape == (2,)
    np.testing.assert_allclose(tok.cpu().numpy(), want.cpu().numpy(), rtol=1e-5, atol=1e-6)
    assert bool((tok[ids2[:, 1:] == 0] == 0).all())
    np.testing.assert_allclose(seq.cpu().numpy(), tok.double().sum(1).cpu().numpy(), rtol=1e-6, atol=1e-6)
    # N = 3 through the fan-out: the oracle's log-probabilities (model tolerance: absolute, on values of a few units)
    seq3, tok3 = m.score_captions(f, k, ids, num_samples=3)
    assert tok3.shape == (6, 6) and seq3.shape == (6,)
    err = np.abs(tok3.cpu().numpy() - ref_tok).max()
    print(f"[score] {dtype}: max |tok_logp - oracle| {err:.3g}")
    assert err < (1e-4 if dtype == torch.float32 else 1e-1)
    assert torch.equal(m.flat_grads, before)                      # forward only: no gradient buffer is written
    with pytest.raises(ValueError):
        m.score_captions(f, k, ids[:5], num_samples=3)


# ---- 7. CaptionTrainer.scst_step ------------------------------------------------------------------------------------------------------------
def _share_reward(tok_id):
    """Toy reward: the share of a caption's tokens (start token excluded, up to its end token) that equal tok_id."""
    def fn(ids, vids):
        a = ids.numpy()
        out = np.zeros(a.shape[:2], np.float32)
        for b in range(a.shape[0]):
            for n in range(a.shape[1]):
                row = [t for t in a[b, n, 1:].tolist() if t != 0]
                out[b, n] = sum(t == tok_id for t in row) / max(len(row), 1)
        return out
    return fn


def test_scst_step(ops):
    from vct_amd.rewards import advantages
    from vct_amd.trainer import CaptionTrainer, FusedAdam
    z, mc, V, cfg, p = _tiny()
    feats, mask = torch.from_numpy(z["feats"]).to(DEV), torch.from_numpy(z["mask"]).to(DEV)
    B, N, kw = feats.shape[0], 4, dict(num_samples=4, max_len=10, seed=7)

    def fresh():
        m = build_model(mc, V, DEV, torch.float32, p)
        m.train()
        return m, CaptionTrainer(m, FusedAdam(m, lr=1e-4))

    def weighted_loss(m, ids, adv):
        seq, tok = m.score_captions(feats, mask, ids.view(B * N, -1), num_samples=N)
        count = int((ids.view(B * N, -1)[:, 1:] != 0).sum())
        return -float((torch.from_numpy(adv.reshape(-1)).to(DEV).double() * seq.double()).sum()) / count

    m, tr = fresh()
    ids0 = m.sample_decode_ids(feats, mask, **kw)
    body = ids0[:, :, 1:].reshape(-1)
    body = body[(body != 0) & (body != 102)]
    tok_id = int(torch.mode(body.cpu())[0])                       # a token the samples do contain: rewards that differ
    reward_fn = _share_reward(tok_id)
    r0 = reward_fn(ids0.cpu(), None)
    assert r0.max() > r0.min()
    adv0 = advantages(r0, "mean_others")
    before = weighted_loss(m, ids0, adv0)
    out = tr.scst_step(feats, mask, reward_fn, **kw)
    assert torch.equal(out["ids"], ids0)                          # the seed reproduces the samples
    assert out["reward_mean"] == pytest.approx(float(r0.mean()), rel=1e-6)
    assert out["baseline_mean"] == pytest.approx(float((r0 - adv0).mean()), rel=1e-5, abs=1e-7)
    assert float(out["loss"]) == pytest.approx(before, rel=1e-4, abs=1e-7)
    after = weighted_loss(m, ids0, adv0)
    print(f"[scst_step] token {tok_id}: weighted loss {before:.6g} -> {after:.6g}")
    assert after < before                                         # Adam's first step is a sign step of size lr: down to first order
    # the same seed from the same weights: the same bits
    m2, tr2 = fresh()
    out2 = tr2.scst_step(feats, mask, reward_fn, **kw)
    assert torch.equal(out2["ids"], out["ids"]) and torch.equal(out2["loss"], out["loss"])
    end = m.caption_param_end                                     # (matching.* is not in the fixture: each model draws its own)
    assert end == m2.caption_param_end and torch.equal(m2.flat_params[:end], m.flat_params[:end])
    # the greedy baseline
    g = m2.greedy_decode_ids(feats, mask, max_len=10)
    base = reward_fn(g.cpu().view(B, 1, -1), None).reshape(B)
    out3 = tr2.scst_step(feats, mask, reward_fn, baseline="greedy", **kw)
    assert np.isfinite(float(out3["loss"])) and out3["ids"].shape[:2] == (B, N)
    assert out3["baseline_mean"] == pytest.approx(float(base.mean()), rel=1e-6, abs=1e-7)
    assert out3["reward_mean"] == pytest.approx(float(reward_fn(out3["ids"].cpu(), None).mean()), rel=1e-6)
