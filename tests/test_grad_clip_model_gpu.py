"""Gradient clipping inside the training step (CaptionTrainer with max_grad_norm / clip_grad_value on the optimizer), on the small
model of tests/test_dist_gpu.py (B = 6, T = 7, S = 9) with dropout on.

The checker of every chain is a second model with the same weights and dropout seed that runs the kernels' forward + backward
only (train_step_kernels*): its gradients, torch's fp32 multiply / clamp on them, and a plain FusedAdam.step().  Bitwise
comparisons throughout (the step is deterministic); the norms are compared with the fp64 norm of the checker's gradients to 1 ulp
of fp32 (tests/test_grad_clip_gpu.py states the error budget)."""
import numpy as np
import pytest
import torch

import grad_clip_ref as R
import vct_oracle as O
from helpers import GradTol, build_model, golden_params, load_golden, model_config_of
from test_dist_gpu import MC, VOCAB

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _model(dtype=torch.bfloat16, seed=7, task="caption"):
    torch.manual_seed(seed)
    mc = dict(MC)
    mc["dropout"] = 0.1
    m = build_model(mc, VOCAB, DEV, dtype)
    m.mode(task)
    m.train()
    m._seed.fill_(1234)
    return m


def _batch(seed, B=6, T=7, S=9):
    g = torch.Generator().manual_seed(seed)
    feats = torch.randn(B, T, 48, generator=g)
    mask = torch.zeros(B, T, dtype=torch.bool); mask[1, T - 2:] = True
    ids = torch.randint(3, VOCAB, (B, S), generator=g); ids[:, 0] = 101; ids[2, S - 3:] = 0
    return feats.to(DEV), mask.to(DEV), ids.to(DEV)


def _owned(m, opt):
    ps = m._ps
    return [n for n in ps.names if ps.params[n].numel() and opt.begin <= ps.offsets[n] and ps.offsets[n] + ps.params[n].numel() <= opt.end]


def _norm64(m, names):
    """(fp64 global norm, fp64 per-parameter norms) of the model's current gradients, by parameter name."""
    sq = [float(m._ps.g[n].double().square().sum()) for n in names]
    return float(np.sqrt(np.sum(np.asarray(sq, np.float64)))), np.sqrt(np.asarray(sq, np.float64))


def _scaled(m, names, coef):
    """The model's flat gradients with every named parameter times coef (fp32, torch): what clipping must leave."""
    want = m.flat_grads.clone()
    ps = m._ps
    for n in names:
        a = ps.offsets[n]
        want[a:a + ps.params[n].numel()] *= coef
    return want


def _check_norms(tr, checker, names, norm64, seg64):
    got_names, seg = tr.grad_norms()
    assert got_names == names
    norm = F32(tr.last_grad_norm.item())
    print(f"[grad-clip-model] norm {norm!r} (fp64 of the checker's gradients {norm64!r}), coef {tr.last_clip_coef.item()!r}")
    assert R.ulps(norm, F32(norm64)) <= 1
    assert (R.ulps(seg.cpu().numpy(), seg64.astype(F32)) <= 1).all()
    assert tr.last_grad_norm.dim() == 0 and tr.last_grad_norm.dtype == torch.float32 and tr.last_grad_norm.is_cuda


def _manual_chain(step_a, backward_b, task="caption"):
    """Model B: kernels' backward only -> its norm picks a threshold that clips; model A: the trainer's step with it.  Then
    A's gradients == fp32(B's * coef_A), norms to 1 ulp, and B scaled + FusedAdam.step() == A's parameters, all bitwise."""
    from vct_amd.trainer import CaptionTrainer, FusedAdam
    b = _model(task=task)
    opt_b = FusedAdam(b, lr=1e-3)
    CaptionTrainer(b, opt_b)                                  # (the same engine settings as A's trainer; it never steps)
    names = _owned(b, opt_b)
    opt_b.sync_hyper()
    b._ps.refresh_shadow()
    backward_b(b)
    norm64, seg64 = _norm64(b, names)
    max_norm = 0.25 * norm64
    a = _model(task=task)
    tr = CaptionTrainer(a, FusedAdam(a, lr=1e-3, max_grad_norm=max_norm))
    assert tr.fuse_adam is False
    out = step_a(tr)
    coef = tr.last_clip_coef.clone()
    assert 0.0 < float(coef) < 1.0 and a.grads_valid
    assert R.same_bits(F32(coef.item()), R.coef_of(F32(tr.last_grad_norm.item()), max_norm))
    _check_norms(tr, b, names, norm64, seg64)
    want = _scaled(b, names, coef)
    assert torch.equal(a.flat_grads, want)
    b.flat_grads.copy_(want)
    opt_b.step()
    torch.cuda.synchronize()
    assert torch.equal(a.flat_params, b.flat_params)
    return out


def test_clipped_step_equals_manual_step():
    batch = _batch(100)
    _manual_chain(lambda tr: tr.step(*batch), lambda b: b.train_step_kernels(*batch))


def test_inactive_clipping_is_the_unfused_step(monkeypatch):
    from vct_amd.trainer import CaptionTrainer, FusedAdam
    a = _model()
    tr = CaptionTrainer(a, FusedAdam(a, lr=1e-3, max_grad_norm=1e9))
    coefs = []
    for k in range(3):
        tr.step(*_batch(100 + k))
        coefs.append(tr.last_clip_coef.clone())
    monkeypatch.setattr(FusedAdam, "fuse_dw_default", False)
    b = _model()
    tr_b = CaptionTrainer(b, FusedAdam(b, lr=1e-3))
    assert tr_b.fuse_adam is False and tr_b.clipper is None and tr_b.last_grad_norm is None
    for k in range(3):
        tr_b.step(*_batch(100 + k))
    torch.cuda.synchronize()
    assert all(float(c) == 1.0 for c in coefs)
    assert torch.equal(a.flat_params, b.flat_params)


@pytest.fixture(scope="module")
def typical_norm():
    """The gradient norm of the first step of the standard model and batch (measured with max_grad_norm = inf: never scales)."""
    from vct_amd.trainer import CaptionTrainer, FusedAdam
    m = _model()
    tr = CaptionTrainer(m, FusedAdam(m, lr=1e-3, max_grad_norm=float("inf")))
    before = m.flat_params.clone()
    tr.step(*_batch(100))
    assert float(tr.last_clip_coef) == 1.0 and not torch.equal(before, m.flat_params)
    n = float(tr.last_grad_norm)
    assert np.isfinite(n) and n > 0
    return n


def _run(executor, thresholds, steps=5):
    from vct_amd.trainer import CaptionTrainer, FusedAdam
    m = _model()
    opt = FusedAdam(m, lr=1e-3, max_grad_norm=thresholds[0])
    tr = CaptionTrainer(m, opt, use_graph=executor == "graph", launch_list=executor == "list")
    rec = []
    for k in range(steps):
        opt.param_groups[0]["max_grad_norm"] = thresholds[k % len(thresholds)]
        loss = tr.step(*_batch(100 + k))
        rec.append(torch.stack([loss.reshape(()), tr.last_grad_norm, tr.last_clip_coef]).clone())
    torch.cuda.synchronize()
    return m.flat_params.clone(), torch.stack(rec), tr


def test_executors_agree_and_follow_the_threshold(typical_norm):
    n = typical_norm
    sched = [0.5 * n, 0.05 * n, 1e9, 0.2 * n, 0.01 * n]
    p0, r0, _ = _run("eager", sched)
    coefs = r0[:, 2].tolist()
    assert coefs[2] == 1.0 and all(0.0 < c < 1.0 for i, c in enumerate(coefs) if i != 2)
    for executor in ("list", "graph"):
        p, r, tr = _run(executor, sched)
        assert tr.use_list or tr.use_graph
        assert len(tr._lists if executor == "list" else tr._graphs) == 1          # one recording served every threshold
        assert torch.equal(r, r0) and torch.equal(p, p0), executor
    p_const, r_const, _ = _run("eager", [0.5 * n])
    assert not torch.equal(p_const, p0)                      # the schedule mattered


def _even_share(ids, vids):
    """Toy reward: the share of even token ids in each caption (pads and the start column excluded)."""
    a = ids.numpy()[:, :, 1:]
    live = a != 0
    return (((a % 2 == 0) & live).sum(-1) / np.maximum(live.sum(-1), 1)).astype(np.float32)


def test_scst_step_clips():
    from vct_amd.rewards import advantages
    feats, mask, _ = _batch(100)
    N, kw = 3, dict(max_len=8, seed=11)

    def backward_b(b):
        ids = b.sample_decode_ids(feats, mask, num_samples=N, **kw)
        r = np.asarray(_even_share(ids.cpu(), None), np.float32)
        assert r.max() > r.min()
        seq_w = torch.from_numpy(np.ascontiguousarray(advantages(r, "mean_others").reshape(-1))).to(DEV)
        b.train_step_kernels_scst(feats, mask, ids.view(feats.shape[0] * N, -1), seq_w, N)
    out = _manual_chain(lambda tr: tr.scst_step(feats, mask, _even_share, num_samples=N, **kw), backward_b)
    assert np.isfinite(float(out["loss"]))


def test_cross_step_clips():
    feats, mask, ids = _batch(100)
    text = torch.randn(feats.shape[0], _model(task="cross").text_encoder.dim, generator=torch.Generator().manual_seed(5)).to(DEV)
    _manual_chain(lambda tr: tr.step(feats, mask, ids, text), lambda b: b.train_step_kernels_cross(feats, mask, ids, text), task="cross")


def test_value_mode_is_torch_clamp():
    from vct_amd.trainer import CaptionTrainer, FusedAdam
    batch = _batch(100)
    b = _model()
    opt_b = FusedAdam(b, lr=1e-3)
    CaptionTrainer(b, opt_b)
    names = _owned(b, opt_b)
    opt_b.sync_hyper()
    b._ps.refresh_shadow()
    b.train_step_kernels(*batch)
    v = 0.1 * float(b.flat_grads[opt_b.begin:opt_b.end].abs().max())
    a = _model()
    tr = CaptionTrainer(a, FusedAdam(a, lr=1e-3, clip_grad_value=v))
    assert tr.fuse_adam is False and tr.last_grad_norm is None and tr.last_clip_coef is None and tr.grad_norms() is None
    tr.step(*batch)
    want = b.flat_grads.clone()
    for n in names:
        x = b._ps.offsets[n]
        want[x:x + b._ps.params[n].numel()].clamp_(-F32(v).item(), F32(v).item())
    assert torch.equal(a.flat_grads, want) and not torch.equal(want, b.flat_grads)
    assert float(a.flat_grads[opt_b.begin:opt_b.end].abs().max()) == F32(v)
    b.flat_grads.copy_(want)
    opt_b.step()
    torch.cuda.synchronize()
    assert torch.equal(a.flat_params, b.flat_params)


def test_grad_norms_against_the_reference_fixture():
    """fp32 compute mode, tests/golden/tiny_train.npz (the reference's own gradients of this batch): the per-parameter norms the
    step reports against the fp64 norms of the fixture's gradients, with test_model_gpu's fp32 gradient tolerance (1e-3, logged
    by helpers.GradTol), and the global norm over the same parameters."""
    from vct_amd.trainer import CaptionTrainer, FusedAdam
    z = load_golden("tiny_train.npz")
    mc = model_config_of(z)
    cfg = O.cfg_from_model_config(mc, int(z["vocab"]))
    m = build_model(mc, int(z["vocab"]), DEV, torch.float32, golden_params(z, cfg))
    m.train()   # dropout is 0.0 in this config
    tr = CaptionTrainer(m, FusedAdam(m, lr=1e-4, max_grad_norm=float("inf")))
    tr.step(torch.from_numpy(z["feats"]).to(DEV), torch.from_numpy(z["mask"]).to(DEV), torch.from_numpy(z["ids"]).to(DEV))
    names, seg = tr.grad_norms()
    seg = dict(zip(names, seg.cpu().numpy().astype(np.float64)))
    ref = {k[len("grad/"):]: float(np.linalg.norm(z[k].astype(np.float64))) for k in z.files if k.startswith("grad/")}
    assert ref and set(ref) <= set(names)
    tol = GradTol("grad_clip_norms_vs_reference", torch.float32, 1e-3)
    for k, r in ref.items():
        tol.add(k, abs(seg[k] - r) / max(r, 1e-30))
    tol.report()
    total = float(np.sqrt(sum(r * r for r in ref.values())))
    mine = float(np.sqrt(sum(seg[k] ** 2 for k in ref)))
    assert abs(mine - total) < 1e-3 * total
    every = float(np.sqrt(sum(v * v for v in seg.values())))      # the global norm is the norm of the per-parameter norms (fp32 each)
    assert abs(float(tr.last_grad_norm) - every) <= 1e-6 * every
    assert float(tr.last_clip_coef) == 1.0


def test_resume_with_clipping(tmp_path, typical_norm):
    from vct_amd import checkpoint as ck
    from vct_amd.trainer import CaptionTrainer, FusedAdam
    thr = 0.3 * typical_norm
    a = _model()
    opt = FusedAdam(a, lr=1e-3, max_grad_norm=thr)
    tr = CaptionTrainer(a, opt)
    for k in range(2):
        tr.step(*_batch(100 + k))
    path = str(tmp_path / "s.pt")
    ck.save_training_state(path, a, opt, None, epoch=0)
    rec_a = []
    for k in range(2, 4):
        tr.step(*_batch(100 + k))
        rec_a.append(torch.stack([tr.last_grad_norm, tr.last_clip_coef]).clone())
    c = _model(seed=8)
    opt_c = FusedAdam(c, lr=5e-2)                            # no clipping, another learning rate: both come from the file
    tr_c = CaptionTrainer(c, opt_c)
    assert tr_c.clipper is None
    ck.load_training_state(path, c, opt_c)
    assert opt_c.param_groups[0]["max_grad_norm"] == thr
    rec_c = []
    for k in range(2, 4):
        tr_c.step(*_batch(100 + k))
        rec_c.append(torch.stack([tr_c.last_grad_norm, tr_c.last_clip_coef]).clone())
    torch.cuda.synchronize()
    assert tr_c.fuse_adam is False and all(0.0 < float(r[1]) < 1.0 for r in rec_a)
    assert torch.equal(torch.stack(rec_a), torch.stack(rec_c))
    end = a.caption_param_end
    assert torch.equal(a.flat_params[:end], c.flat_params[:end])
