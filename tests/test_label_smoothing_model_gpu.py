"""Label smoothing through the model (GPU), on the tiny configuration of tests/test_model_gpu.py (d 64, V 131, B 3, ragged pads):
loss, gradients and one Adam step against oracle/torch_ref.py with the smoothed criterion; the three executors bitwise with the NLL /
accuracy by-products; smoothing 0 and an absent key are the same model and never reach the new entry point; loss_stats at smoothing 0
changes no bit of loss or gradient; the self-critical step and score_captions ignore the smoothing; val_epoch."""
import copy
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import vct_oracle as O
from helpers import GradTol, build_model, golden_params, load_golden, model_config_of, rel

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _tiny(alpha=None, eps=None, dropout=None, **dec):
    z = load_golden("tiny_train.npz")
    mc = copy.deepcopy(model_config_of(z))
    if alpha is not None:
        mc["caption_decoder"]["sce_loss_alpha"] = alpha
    if eps is not None:
        mc["caption_decoder"]["label_smoothing"] = eps
    if dropout is not None:
        mc["dropout"] = dropout
    mc["caption_decoder"].update(dec)
    cfg = O.cfg_from_model_config(mc, int(z["vocab"]))
    return z, mc, cfg, golden_params(z, cfg)


def _batch(z):
    return torch.from_numpy(z["feats"]).to(DEV), torch.from_numpy(z["mask"]).to(DEV), torch.from_numpy(z["ids"]).to(DEV)


def _smoothed_loss_fn(eps):
    """oracle/torch_ref.py: _Decoder.loss_fn with the CE term smoothed (the RCE term as it is)."""
    def loss_fn(self, logits, labels):
        ce = F.cross_entropy(logits, labels, ignore_index=self.pad_id, label_smoothing=eps)
        if self.alpha == 1.0:
            return ce
        p = F.softmax(logits, dim=1).clamp(min=1e-7, max=1.0)
        onehot = F.one_hot(labels, self.vocab).float().clamp(min=1e-4, max=1.0)
        rce = -(p * onehot.log()).sum(dim=1)
        return self.alpha * ce + (1.0 - self.alpha) * rce.mean()
    return loss_fn


def _torch_reference(z, cfg, p, eps, lr):
    """(loss, grads by name, parameters after one Adam step, NLL, token accuracy) of the torch module graph on the CPU, fp32."""
    import torch_ref as TR
    torch.manual_seed(0)
    ref = TR.RefCaptionModel(cfg, dropout=0.0)
    ref.load_oracle_params(p)
    ref.cap_decoder.loss_fn = types.MethodType(_smoothed_loss_fn(eps), ref.cap_decoder)
    ref.train()
    ids = torch.from_numpy(z["ids"])
    logits, loss = ref(torch.from_numpy(z["feats"]), torch.from_numpy(z["mask"]), ids)
    opt = torch.optim.Adam(ref.parameters(), lr=lr, betas=(0.9, 0.999))
    opt.zero_grad()
    loss.backward()
    grads = {k: q.grad.detach().clone() for k, q in ref.named_parameters() if q.grad is not None}
    opt.step()
    after = {k: q.detach().clone() for k, q in ref.named_parameters()}
    lg, lab = logits.detach().reshape(-1, logits.shape[-1]), ids[:, 1:].reshape(-1)
    valid = lab != cfg["pad_id"]
    nll = F.cross_entropy(lg, lab, ignore_index=cfg["pad_id"])
    acc = (lg[valid].gather(1, lab[valid][:, None])[:, 0] == lg[valid].max(1).values).float().mean()
    return float(loss), grads, after, float(nll), float(acc), int(valid.sum())


@pytest.mark.parametrize("alpha", [1.0, 0.5])
@pytest.mark.parametrize("dtype,tl,tg", [(torch.float32, 1e-5, 1e-3), (torch.bfloat16, 2e-3, 3e-2)], ids=["fp32", "bf16"])
def test_loss_gradients_and_adam_step_vs_torch_reference(dtype, tl, tg, alpha):
    eps, lr = 0.1, 1e-4
    z, mc, cfg, p = _tiny(alpha=alpha, eps=eps)
    ref_loss, ref_g, ref_after, ref_nll, ref_acc, count = _torch_reference(z, cfg, p, eps, lr)
    assert ref_nll != pytest.approx(ref_loss, rel=1e-3)            # the smoothing is visible in the criterion
    m = build_model(mc, int(z["vocab"]), DEV, dtype, p)
    m.train()                                                       # dropout 0 in this configuration
    feats, mask, ids = _batch(z)
    opt = torch.optim.Adam(filter(lambda q: q.requires_grad, m.parameters()), lr=lr, betas=(0.9, 0.999))
    loss = m([feats], [mask], ids)
    opt.zero_grad()
    loss.backward()
    print(f"[ls-model] {dtype} alpha={alpha}: loss {float(loss)!r} reference {ref_loss!r}")
    assert abs(float(loss) - ref_loss) < tl * abs(ref_loss)
    stats = m.cap_decoder._engine().last_loss_stats
    assert stats is not None and abs(float(stats[0]) - ref_nll) < tl * abs(ref_nll)
    # an argmax may flip on a near-tie in bf16: one token of the batch
    assert abs(float(stats[1]) - ref_acc) <= (0.0 if dtype == torch.float32 else 1.0 / count) + 1e-6
    named = dict(m.named_parameters())
    tol = GradTol(f"label_smoothing_vs_torch_reference alpha={alpha}", dtype, tg)
    for k, g in ref_g.items():
        tol.add(k, rel(named[k].grad, g))
    tol.report()
    assert float(named["cap_decoder.tgt_to_emb.weight"].grad[0].abs().sum()) == 0.0
    opt.step()
    after = GradTol(f"label_smoothing_adam_step_vs_torch_reference alpha={alpha}", dtype, tg)
    for k, g in ref_g.items():
        after.add(k, rel(named[k], ref_after[k]))
        if dtype == torch.float32:                                  # the update itself, where the gradient is not rounding noise
            upd_ref = ref_after[k].double().numpy() - p[k]
            upd = named[k].detach().cpu().double().numpy() - p[k]
            big = np.abs(g.numpy()) > 1e-5
            assert np.abs(upd - upd_ref)[big].max(initial=0) < 5e-6, k
    after.report()


def _run_executor(executor, steps=3):
    from vct_amd.trainer import CaptionTrainer, FusedAdam
    z, mc, cfg, p = _tiny(alpha=0.5, eps=0.1, dropout=0.3)
    torch.manual_seed(5)
    m = build_model(mc, int(z["vocab"]), DEV, torch.bfloat16, p)
    m.train()
    tr = CaptionTrainer(m, FusedAdam(m, lr=1e-3), use_graph=executor == "graph", launch_list=executor == "list")
    feats, mask, ids = _batch(z)
    rec = []
    for _ in range(steps):
        loss = tr.step(feats, mask, ids)
        assert tr.last_nll is not None and tr.last_nll.dim() == 0 and tr.last_token_acc.dim() == 0
        rec.append(torch.stack([loss.reshape(()), tr.last_nll, tr.last_token_acc]).clone())
    torch.cuda.synchronize()
    return torch.stack(rec), m.flat_params.clone(), tr


def test_executors_are_bitwise_equal_with_the_by_products():
    r0, p0, tr0 = _run_executor("eager")
    assert not (tr0.use_list or tr0.use_graph)
    assert bool(torch.isfinite(r0).all()) and bool((r0[:, 1] != r0[:, 0]).all())       # the NLL is not the smoothed criterion
    assert bool((r0[:, 2] >= 0).all()) and bool((r0[:, 2] <= 1).all())
    assert not torch.equal(r0[0], r0[1])                             # the replays rewrite the by-products, step after step
    for executor in ("list", "graph"):
        r, p, tr = _run_executor(executor)
        assert tr.use_list if executor == "list" else tr.use_graph
        assert torch.equal(r, r0) and torch.equal(p, p0), executor


def test_by_products_equal_the_reference_values_on_the_trainer():
    """Dropout 0: the trainer's last_nll / last_token_acc against the torch reference (eager and launch list)."""
    from vct_amd.trainer import CaptionTrainer, FusedAdam
    z, mc, cfg, p = _tiny(alpha=1.0, eps=0.1)
    ref_loss, _, _, ref_nll, ref_acc, count = _torch_reference(z, cfg, p, 0.1, 1e-4)
    for launch_list in (False, True):
        m = build_model(mc, int(z["vocab"]), DEV, torch.float32, p)
        m.train()
        tr = CaptionTrainer(m, FusedAdam(m, lr=1e-12), launch_list=launch_list)
        for _ in range(3 if launch_list else 1):                     # lr 1e-12: every step sees the same weights to fp32 resolution; the third is a replay
            loss = tr.step(*_batch(z))
        assert abs(float(loss) - ref_loss) < 1e-5 * ref_loss
        assert abs(float(tr.last_nll) - ref_nll) < 1e-5 * ref_nll and float(tr.last_token_acc) == pytest.approx(ref_acc, abs=1e-6)


def _step_bits(mc, z, p, loss_stats=None, dtype=torch.bfloat16):
    torch.manual_seed(5)
    m = build_model(mc, int(z["vocab"]), DEV, dtype, p)
    m.train()
    if loss_stats is not None:
        m.cap_decoder.loss_stats = loss_stats
    loss = m.train_step_kernels(*_batch(z)).clone()
    return loss, m.flat_grads.clone(), m


def test_zero_smoothing_is_the_absent_key_and_never_reaches_the_new_entry_point(monkeypatch):
    from vct_amd import ops

    def boom(*a, **kw):
        raise AssertionError("ops.sce_loss_ls reached without label smoothing or loss_stats")
    monkeypatch.setattr(ops, "sce_loss_ls", boom)
    for alpha in (1.0, 0.5):
        z, mc_absent, _, p = _tiny(alpha=alpha, dropout=0.3)
        _, mc_zero, _, _ = _tiny(alpha=alpha, eps=0, dropout=0.3)
        assert "label_smoothing" not in mc_absent["caption_decoder"] and mc_zero["caption_decoder"]["label_smoothing"] == 0
        l0, g0, m0 = _step_bits(mc_absent, z, p)
        l1, g1, m1 = _step_bits(mc_zero, z, p)
        assert torch.equal(l0, l1) and torch.equal(g0, g1)
        assert m0.cap_decoder._engine().last_loss_stats is None and m1.cap_decoder._engine().last_loss_stats is None
    z, mc, _, p = _tiny(eps=0.1)
    with pytest.raises(AssertionError, match="sce_loss_ls reached"):
        _step_bits(mc, z, p)                                         # and with smoothing the step does go there


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_loss_stats_at_zero_smoothing_changes_no_bit(dtype):
    for alpha in (1.0, 0.5):
        z, mc, cfg, p = _tiny(alpha=alpha, dropout=0.3)
        l0, g0, m0 = _step_bits(mc, z, p, dtype=dtype)
        l1, g1, m1 = _step_bits(mc, z, p, loss_stats=True, dtype=dtype)
        assert torch.equal(l0.view(torch.int32), l1.view(torch.int32)) and torch.equal(g0.view(torch.int32), g1.view(torch.int32))
        stats = m1.cap_decoder._engine().last_loss_stats
        assert m0.cap_decoder._engine().last_loss_stats is None and stats is not None
        if alpha == 1.0:
            assert float(stats[0]) == float(l1)                      # the un-smoothed CE is the NLL


def test_trainer_loss_stats_switch_drops_recordings():
    from vct_amd.trainer import CaptionTrainer, FusedAdam
    z, mc, cfg, p = _tiny(alpha=1.0)
    m = build_model(mc, int(z["vocab"]), DEV, torch.bfloat16, p)
    m.train()
    tr = CaptionTrainer(m, FusedAdam(m, lr=1e-3), launch_list=True)
    for _ in range(2):
        tr.step(*_batch(z))
    assert tr.last_nll is None and len(tr._lists) == 1
    m.cap_decoder.loss_stats = True
    loss = tr.step(*_batch(z))
    assert tr.last_nll is not None and float(tr.last_nll) == float(loss)
    loss = tr.step(*_batch(z))                                       # a replay of the new recording
    assert float(tr.last_nll) == float(loss)
    tr2 = CaptionTrainer(m, FusedAdam(m, lr=1e-3), loss_stats=False)
    tr2.step(*_batch(z))
    assert m.cap_decoder.loss_stats is False and tr2.last_nll is None


def _even_share(ids, vids):
    a = ids.numpy()[:, :, 1:]
    live = a != 0
    return (((a % 2 == 0) & live).sum(-1) / np.maximum(live.sum(-1), 1)).astype(np.float32)


def test_scst_step_and_score_captions_ignore_the_smoothing():
    from vct_amd.trainer import CaptionTrainer, FusedAdam
    outs = []
    for eps in (None, 0.1):
        z, mc, cfg, p = _tiny(alpha=0.5, eps=eps)
        torch.manual_seed(5)
        m = build_model(mc, int(z["vocab"]), DEV, torch.bfloat16, p)
        feats, mask, ids = _batch(z)
        seq, tok = m.score_captions([feats], [mask], ids)
        m.train()
        tr = CaptionTrainer(m, FusedAdam(m, lr=1e-3))
        out = tr.scst_step(feats, mask, _even_share, num_samples=3, max_len=6, seed=11)
        assert tr.last_nll is None
        outs.append((seq.clone(), tok.clone(), torch.as_tensor(out["loss"]).reshape(-1).clone(), m.flat_params.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_val_epoch_returns_the_smoothed_criterion_and_the_nll_on_request():
    from vct_amd.evaluate import val_epoch
    z, mc, cfg, p = _tiny(alpha=1.0, eps=0.1)
    ref_loss, _, _, ref_nll, ref_acc, _ = _torch_reference(z, cfg, p, 0.1, 1e-4)
    m = build_model(mc, int(z["vocab"]), DEV, torch.float32, p)
    feats, mask, ids = _batch(z)
    loader = [([feats], [mask], ids, None)] * 2
    v = val_epoch(m, loader)
    assert isinstance(v, float) and abs(v - ref_loss) < 1e-5 * ref_loss
    v2, stats = val_epoch(m, loader, with_stats=True)
    assert v2 == v and abs(stats["nll"] - ref_nll) < 1e-5 * ref_nll and stats["token_acc"] == pytest.approx(ref_acc, abs=1e-6)
    # without smoothing the switch is on for the epoch only
    z, mc0, cfg, p = _tiny(alpha=1.0)
    m0 = build_model(mc0, int(z["vocab"]), DEV, torch.float32, p)
    v0, s0 = val_epoch(m0, loader, with_stats=True)
    assert s0["nll"] == pytest.approx(v0, rel=1e-6) and m0.cap_decoder.loss_stats is False
    assert val_epoch(m0, loader) == v0
