"""The video-text matching task on the GPU: the loss kernels against the float64 restatement (tests/matching_ref.py), the
aggregation-row kernels, and parity of the match / cross steps with the reference (tests/golden/matching_*.npz,
tools/make_golden_matching.py) through both the autograd path with torch.optim.Adam and CaptionTrainer with FusedAdam.

Tolerances: the kernels are fp32 against fp64 -- loss 1e-5 relative, dvid and sim 1e-4 relative-Frobenius,
|dtemp - ref| <= 1e-5 * sum |terms|, 1e-7 absolute where the reference is exactly 0 (B = 1).  Fixtures as tests/test_multimodal_gpu.py:
fp32 loss 1e-5, activations 1e-4, gradients 1e-3, Adam updates 5e-6 on entries whose gradient exceeds 1e-5; bf16 loss 2e-3,
gradients 3e-2."""
import json

import numpy as np
import pytest
import torch

import matching_ref as R
from helpers import GradTol, build_model, load_golden, model_config_of, rel

pytestmark = pytest.mark.gpu
DEV = "cuda"
V = 131


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- vct_match_loss ------------------------------------------------------------------------------------------------------------------
SHAPES = sorted(set([(B, Dt) for B in (1, 2, 5, 64, 67, 256) for Dt in (20, 768)] + [(67, Dt) for Dt in (16, 20, 512, 768)]))
TEMPS = [("CSL", "none", None), ("CSL", "exp", 0.07), ("CSL", "exp", 2.5), ("CSL_WDS", "div", 0.5), ("CSL_WDS", "div", 0.05)]


def _run_loss(text, vid, kind, tkind, temp, backward=True, want_sim=True):
    from vct_amd import ops
    B, Dt = text.shape
    ws = torch.empty(ops.match_loss_workspace_bytes(B, Dt) // 4, dtype=torch.float32, device=DEV)
    loss = torch.full((1,), float("nan"), device=DEV)
    dvid = torch.full((B, Dt + 4), float("nan"), device=DEV)[:, :Dt] if backward else None      # a leading dimension of its own
    dtemp = torch.full((1,), float("nan"), device=DEV) if backward and temp is not None else None
    sim = torch.full((B, B), float("nan"), device=DEV) if want_sim else None
    t = torch.tensor([temp], dtype=torch.float32, device=DEV) if temp is not None else None
    ops.match_loss(text, vid, loss, ws, kind=kind, temp=t, temp_kind=tkind, dvid=dvid, dtemp=dtemp, sim=sim)
    return loss, dvid, dtemp, sim


@pytest.mark.parametrize("B,Dt", SHAPES)
def test_match_loss_vs_fp64(B, Dt):
    rng = np.random.default_rng(1000 * B + Dt)
    tn, vn = rng.standard_normal((B, Dt)).astype(np.float32), rng.standard_normal((B, Dt)).astype(np.float32)
    # strided rows: views into wider buffers (leading dimensions Dt + 8 and Dt + 12)
    text = torch.zeros(B, Dt + 8, device=DEV)[:, :Dt]
    vid = torch.zeros(B, Dt + 12, device=DEV)[:, :Dt]
    text.copy_(_dev(tn))
    vid.copy_(_dev(vn))
    for kind, tkind, temp in TEMPS:
        ref = R.head(tn, vn, kind, temp)
        loss, dvid, dtemp, sim = _run_loss(text, vid, kind, tkind, temp)
        got = dict(loss=float(loss), dvid=dvid.double().cpu().numpy(), sim=sim.double().cpu().numpy(),
                   dtemp=float(dtemp) if dtemp is not None else None)
        tag = (B, Dt, kind, temp)
        e_sim = rel(got["sim"], ref["sim"])
        print("[match-loss]", tag, "loss", got["loss"], ref["loss"], "sim", e_sim, end=" ")
        assert e_sim < 1e-4, tag
        if B == 1:      # the reference is exactly 0
            print("abs", abs(got["loss"]), np.abs(got["dvid"]).max(), got["dtemp"])
            assert abs(got["loss"]) <= 1e-7 and np.abs(got["dvid"]).max() <= 1e-7, tag
            assert got["dtemp"] is None or abs(got["dtemp"]) <= 1e-7, tag
        else:
            e_dv = rel(got["dvid"], ref["dvid"])
            print("dvid", e_dv, "dtemp", got["dtemp"], ref["dtemp"], ref["dtemp_abs"])
            assert abs(got["loss"] - ref["loss"]) < 1e-5 * abs(ref["loss"]), tag
            assert e_dv < 1e-4, tag
            if temp is not None:
                assert abs(got["dtemp"] - ref["dtemp"]) <= 1e-5 * ref["dtemp_abs"], tag
        assert np.isfinite(got["dvid"]).all() and np.isfinite(got["sim"]).all()
        # two calls agree bitwise; forward only (no dvid) returns the same loss bits
        loss2, dvid2, dtemp2, sim2 = _run_loss(text, vid, kind, tkind, temp)
        assert torch.equal(loss, loss2) and torch.equal(dvid, dvid2) and torch.equal(sim, sim2), tag
        assert dtemp is None or torch.equal(dtemp, dtemp2), tag
        loss3, _, _, sim3 = _run_loss(text, vid, kind, tkind, temp, backward=False)
        assert torch.equal(loss, loss3) and torch.equal(sim, sim3), tag
        loss4, _, _, _ = _run_loss(text, vid, kind, tkind, temp, backward=False, want_sim=False)
        assert torch.equal(loss, loss4), tag


def test_match_loss_refuses_unsupported_shapes_in_python():
    from vct_amd import ops
    t = torch.zeros(257, 16, device=DEV)
    with pytest.raises(ValueError, match="outside the kernels' range"):
        ops.match_loss(t, t, torch.zeros(1, device=DEV), torch.zeros(16, device=DEV))
    t = torch.zeros(4, 18, device=DEV)
    with pytest.raises(ValueError, match="outside the kernels' range"):
        ops.match_loss(t, t, torch.zeros(1, device=DEV), torch.zeros(16, device=DEV))


# ---- vct_match_agg ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("Te,d", [(1, 64), (6, 64), (10, 768), (6, 768)])
def test_match_agg_both_ways(dtype, Te, d):
    from vct_amd import ops
    B = 5
    torch.manual_seed(Te * 1000 + d)
    mem = torch.randn(B * Te, d, device=DEV).to(dtype)
    agg = torch.full((B, d), float("nan"), device=DEV)
    ops.match_agg_fwd(mem, agg, B, Te)
    assert torch.equal(agg, mem.view(B, Te, d)[:, 0].float())
    dagg = torch.randn(B, d, device=DEV)
    # "empty": the buffer holds nothing yet (NaN here) and must not be read; beta = 0 hands dagg through exactly
    dmem = torch.full((B * Te, d), float("nan"), device=DEV).to(dtype)
    ops.match_agg_bwd(dmem, dagg, B, Te, 0.0, empty=True)
    want = torch.zeros(B, Te, d, device=DEV)
    want[:, 0] = dagg
    assert torch.equal(dmem.view(B, Te, d), want.to(dtype))
    # beta = 0.3 on a filled buffer: fp32 products rounded separately, one add, one rounding to the dtype
    old = torch.randn(B * Te, d, device=DEV).to(dtype)
    dmem = old.clone()
    ops.match_agg_bwd(dmem, dagg, B, Te, 0.3)
    beta = torch.tensor(0.3, dtype=torch.float32, device=DEV)
    want = (beta * old.float()).view(B, Te, d)
    want[:, 0] = want[:, 0] + (1.0 - beta) * dagg
    assert torch.equal(dmem.view(B, Te, d), want.to(dtype))


def test_scale_and_axpby():
    from vct_amd import ops
    x = torch.randn(64 * 37 + 3, device=DEV)
    y = x.clone()
    ops.scale(y[:64 * 37 + 2], 0.3)
    assert torch.equal(y[:-1], x[:-1] * torch.tensor(0.3, device=DEV)) and torch.equal(y[-1:], x[-1:])
    a, b = torch.randn(5, device=DEV), torch.randn(5, device=DEV)
    out = torch.empty(5, device=DEV)
    ops.axpby(out, a, 0.3, b, 0.7)
    assert torch.equal(out, torch.tensor(0.3, device=DEV) * a + torch.tensor(0.7, device=DEV) * b)
    ops.axpby(out, a, 1.0)
    assert torch.equal(out, a)


# ---- the reference's numbers -------------------------------------------------------------------------------------------------------------
def _case(name, dtype=torch.float32, **over):
    z = load_golden(f"matching_{name}.npz")
    mc = dict(model_config_of(z), **over)
    m = build_model(mc, V, DEV, dtype, R.matching_params(mc, V, int(z["param_seed"])))
    n = len(mc["modal_shape"])
    feats, masks = [_dev(z[f"feats{i}"]) for i in range(n)], [_dev(z[f"mask{i}"]) for i in range(n)]
    return z, m, feats, masks, _dev(z["ids"]), _dev(z["text_feats"])


def _check_grads(m, z, name, dtype, bound):
    named = dict(m.named_parameters())
    tol = GradTol(name, dtype, bound)
    gk = [k[len("grad/"):] for k in z.files if k.startswith("grad/")]
    for k in gk:
        tol.add(k, rel(named[k].grad, z["grad/" + k]))
    tol.report()
    return gk, named


def _check_adam(named, before, z, za, gk):
    for k in gk:
        upd_ref = za["adam1/" + k].astype(np.float64) - before[k]
        upd = named[k].detach().cpu().numpy().astype(np.float64) - before[k]
        big = np.abs(z["grad/" + k]) > 1e-5
        assert np.abs(upd - upd_ref)[big].max(initial=0) < 5e-6, k


@pytest.mark.parametrize("name", ["P", "L", "N", "W_fixed", "W_learned"])
def test_match_task_vs_reference_autograd(name):
    z, m, feats, masks, ids, text = _case(name)
    m.mode("match")
    m.train()
    _mem, _gmask, agg = m.video_encoder(feats, masks)
    assert rel(agg, z["agg"]) < 1e-4
    assert rel(m.matching.similarity(text, agg.float().contiguous()), z["sim"]) < 1e-4
    opt = torch.optim.Adam(filter(lambda q: q.requires_grad, m.parameters()), lr=1e-4, betas=(0.9, 0.999))
    loss = m(feats, masks, ids, text_feats=text)
    assert abs(float(loss.detach()) - float(z["loss"])) < 1e-5 * float(z["loss"])
    opt.zero_grad()
    loss.backward()
    gk, named = _check_grads(m, z, f"matching_{name}_autograd", torch.float32, 1e-3)
    assert sorted(k for k, q in named.items() if q.grad is None) == sorted(json.loads(str(z["no_grad"])))
    assert all(q.grad is None for q in m.cap_decoder.parameters())
    before = {k: q.detach().cpu().numpy().astype(np.float64) for k, q in named.items()}
    dec_before = {k: q.detach().clone() for k, q in named.items() if k.startswith("cap_decoder.")}
    opt.step()
    _check_adam(named, before, z, z, gk)
    assert all(torch.equal(named[k].detach(), v) for k, v in dec_before.items())


@pytest.mark.parametrize("name", ["P", "L", "N", "W_fixed", "W_learned"])
def test_match_task_vs_reference_trainer(name):
    from vct_amd.trainer import CaptionTrainer, FusedAdam
    z, m, feats, masks, ids, text = _case(name)
    m.mode("match")
    m.train()
    opt = FusedAdam(m, lr=1e-4, betas=(0.9, 0.999))
    tr = CaptionTrainer(m, opt)
    assert not tr.fuse_adam
    named = dict(m.named_parameters())
    before = {k: q.detach().cpu().numpy().astype(np.float64) for k, q in named.items()}
    dec_before = {k: q.detach().clone() for k, q in named.items() if k.startswith("cap_decoder.")}
    f, mk = m._video_inputs(feats, masks)
    loss = tr.step(f, mk, None, text)
    assert abs(float(loss) - float(z["loss"])) < 1e-5 * float(z["loss"])
    assert m.grads_valid
    gk = [k[len("grad/"):] for k in z.files if k.startswith("grad/")]
    for k in gk:
        assert rel(m._ps.g[k], z["grad/" + k]) < 1e-3, k
    _check_adam(named, before, z, z, gk)
    assert all(torch.equal(named[k].detach(), v) for k, v in dec_before.items())
    with pytest.raises(ValueError, match="optimizer was built"):
        m.mode("cross")
        tr.step(f, mk, ids, text)


def test_cross_task_vs_reference():
    from vct_amd.trainer import CaptionTrainer, FusedAdam
    z, m, feats, masks, ids, text = _case("X")
    za = load_golden("matching_X_adam.npz")
    m.mode("cross")
    m.train()
    opt = torch.optim.Adam(filter(lambda q: q.requires_grad, m.parameters()), lr=1e-4, betas=(0.9, 0.999))
    loss, cap, match = m(feats, masks, ids, text_feats=text)
    assert not cap.requires_grad and not match.requires_grad and loss.requires_grad
    for got, key in ((loss, "loss"), (cap, "cap_loss"), (match, "match_loss")):
        assert abs(float(got.detach()) - float(z[key])) < 1e-5 * float(z[key]), key
    opt.zero_grad()
    loss.backward()
    gk, named = _check_grads(m, z, "matching_X_autograd", torch.float32, 1e-3)
    assert all(q.grad is not None for q in named.values())
    before = {k: q.detach().cpu().numpy().astype(np.float64) for k, q in named.items()}
    opt.step()
    _check_adam(named, before, z, za, gk)
    # the trainer with FusedAdam on a fresh model: same numbers
    z, m, feats, masks, ids, text = _case("X")
    m.mode("cross")
    m.train()
    tr = CaptionTrainer(m, FusedAdam(m, lr=1e-4, betas=(0.9, 0.999)))
    named = dict(m.named_parameters())
    before = {k: q.detach().cpu().numpy().astype(np.float64) for k, q in named.items()}
    out = tr.step(feats, masks, ids, text)
    for got, key in zip(out, ("loss", "cap_loss", "match_loss")):
        assert abs(float(got) - float(z[key])) < 1e-5 * float(z[key]), key
    assert m.grads_valid
    for k in gk:
        assert rel(m._ps.g[k], z["grad/" + k]) < 1e-3, k
    _check_adam(named, before, z, za, gk)


def test_cross_task_at_the_ends_of_beta():
    """loss_beta 1: the caption task's gradients of the same batch, nothing for matching.*; loss_beta 0: the match task's gradients
    for the encoder and matching.*, zeros for the decoder.  Within 1e-6 relative per tensor."""
    z, m, feats, masks, ids, text = _case("X")
    m.train()
    names = m._ps.names
    m.mode("caption")
    cap_loss = m.train_step_kernels(feats, masks, ids).clone()
    g_cap = {k: m._ps.g[k].clone() for k in names}
    m.mode("match")
    match_loss = m.train_step_kernels_match(feats, masks, text).clone()
    g_match = {k: m._ps.g[k].clone() for k in names}
    m.mode("cross")
    m.loss_beta = 1.0
    loss, cap, match = (t.clone() for t in m.train_step_kernels_cross(feats, masks, ids, text))
    assert torch.equal(loss, cap_loss) and torch.equal(cap, cap_loss) and torch.equal(match, match_loss)
    for k in names:
        if k.startswith("matching."):
            assert not m._ps.g[k].any(), k
        else:
            assert rel(m._ps.g[k], g_cap[k]) < 1e-6, k
    m.loss_beta = 0.0
    loss, cap, match = (t.clone() for t in m.train_step_kernels_cross(feats, masks, ids, text))
    assert torch.equal(loss, match_loss) and torch.equal(cap, cap_loss)
    for k in names:
        if k.startswith("cap_decoder."):
            assert not m._ps.g[k].any(), k
        else:
            assert rel(m._ps.g[k], g_match[k]) < 1e-6, k


@pytest.mark.parametrize("name,task", [("N", "match"), ("X", "cross")])
def test_bf16_step_vs_reference(name, task):
    """bf16 compute mode: the encoder (and decoder) run in bf16, the head in fp32 on the bf16 memory's aggregation rows."""
    from vct_amd.trainer import CaptionTrainer, FusedAdam
    z, m, feats, masks, ids, text = _case(name, torch.bfloat16)
    m.mode(task)
    m.train()
    tr = CaptionTrainer(m, FusedAdam(m, lr=1e-4, betas=(0.9, 0.999)))
    out = tr.step(feats, masks, ids, text)
    keys = ("loss", "cap_loss", "match_loss") if task == "cross" else ("loss",)
    for got, key in zip(out if task == "cross" else (out,), keys):
        print("[match-bf16]", name, key, float(got), float(z[key]))
        assert abs(float(got) - float(z[key])) < 2e-3 * float(z[key]), key
    tol = GradTol(f"matching_{name}_bf16", torch.bfloat16, 3e-2)
    for k in [k[len("grad/"):] for k in z.files if k.startswith("grad/")]:
        tol.add(k, rel(m._ps.g[k], z["grad/" + k]))
    tol.report()


def test_epoch_loops_and_eval():
    """train_epoch / val_epoch in the match and cross modes (text features from text_feats_fn or an installed backend)."""
    from vct_amd.evaluate import val_epoch
    from vct_amd.trainer import FusedAdam, train_epoch
    z, m, feats, masks, ids, text = _case("X")
    loader = [([f.cpu() for f in feats], [k.cpu() for k in masks], ids.cpu(), ["a", "b", "c"])] * 2
    m.mode("cross")
    got = val_epoch(m, loader, mode="cross", text_feats_fn=lambda caps, vids: text)
    assert isinstance(got, tuple) and len(got) == 3
    for g, key in zip(got, ("loss", "cap_loss", "match_loss")):      # eval mode, dropout 0 in the fixture: the same numbers
        assert abs(g - float(z[key])) < 1e-5 * float(z[key]), key
    m.text_encoder.backend = lambda caps: text
    m.mode("match")
    got = val_epoch(m, loader, mode="match")
    assert isinstance(got, float) and abs(got - float(z["match_loss"])) < 1e-5 * float(z["match_loss"])
    first = train_epoch(m, FusedAdam(m, lr=1e-4), loader, mode="match")
    assert isinstance(first, float) and first < float(z["match_loss"]) * (1 + 1e-5)      # two steps on one batch: the second is lower
    m.mode("cross")
    out = train_epoch(m, FusedAdam(m, lr=1e-4), loader, mode="cross", text_feats_fn=lambda caps, vids: text)
    assert isinstance(out, tuple) and len(out) == 3 and all(np.isfinite(out))
    assert abs(out[0] - (0.3 * out[1] + 0.7 * out[2])) < 1e-5 * out[0]
    # caption behaviour and return type are unchanged
    m.mode("caption")
    assert isinstance(val_epoch(m, loader), float)
