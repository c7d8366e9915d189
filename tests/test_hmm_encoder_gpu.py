"""The hierarchical multi-modal encoder (video_encoder.type "hmme") on the GPU: the vct_hmm_mix_* kernels against torch.where / torch
sums on the same operands (bitwise), parity with the reference's HMMEncoder (tests/golden/hmm_*.npz, tools/make_golden_hmm_encoder.py),
decode, the three executors, launch counts, bit-exact resume and the exchange path.

Tolerances: parity as tests/test_encoder_variants_gpu.py (fp32 loss 1e-5 rel, activations 1e-4, gradients 1e-3; bf16 loss 2e-3,
activations 2e-2, gradients 3e-2 through helpers.GradTol).  bf16 with 'max' (case B): unify.*.weight gradients are logged, not
asserted, for the reason in that file's header (a near-tied maximum may move to another row after rounding to bf16).
agg_feats [B] is a SUM over the n * d elements of the streams' first memory rows, so it has no relative bound of its own (the terms
cancel): |agg - ref|_2 <= sqrt(n d) x |memory - ref|_F by Cauchy-Schwarz per sample, and the memory's error is bounded by the
activation tolerance tl x |ref memory|_F -- that product is the bound used.
Exchange path at world size 1: bitwise, as tests/test_executor_gpu.py::test_own_rccl_communicator_world1_step_is_the_plain_step
asserts for `mme` (torch.equal on losses and flat parameters)."""
import math

import numpy as np
import pytest
import torch

from encvar_ref import encvar_config, encvar_params
from helpers import GradTol, build_model, load_golden, model_config_of, rel
from hmm_ref import hmm_config, hmm_params
from mm_ref import mm_batch

pytestmark = pytest.mark.gpu
DEV = "cuda"
EMB = "video_encoder.temp_emb.embedding.weight"
OPTS = dict(aggregation="max", temporal="embedding", do_norm=True)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- kernels ---------------------------------------------------------------------------------------------------------------
def _takes(Ts, g):
    """Three per-layer tables over S = sum(T_i + 1) rows; whole streams continue or restart, and every table is mixed when S allows."""
    rows = []
    for k in range(3):
        per = [(int(torch.randint(0, 2, (1,), generator=g)) if len(Ts) > 1 else 0) for _ in Ts]
        if len(Ts) > 1 and len(set(per)) == 1:
            per[k % len(Ts)] ^= 1
        t = torch.cat([torch.full((n + 1,), v, dtype=torch.uint8) for n, v in zip(Ts, per)])
        if len(Ts) == 1:
            t[k % len(t)] = 1          # one stream: rows split by hand (the kernel only sees a table)
        rows.append(t)
    return [t.to(DEV) for t in rows]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("Ts,B,d", [((1,), 1, 64), ((3, 2), 3, 64), ((4, 1, 2), 2, 64), ((3, 2), 3, 72)])
def test_mix_kernels_bitwise(dtype, Ts, B, d):
    from vct_amd import ops
    g = torch.Generator(device="cpu").manual_seed(17 * len(Ts) + B + d)
    S = sum(t + 1 for t in Ts)
    takes = _takes(Ts, g)

    def rnd():
        return torch.randn(B * S, d, generator=g).to(DEV).to(dtype)

    def poison(v, dt=dtype):
        return torch.full((B * S, d), v, device=DEV).to(dt)
    # forward: a bitwise copy of the chosen row
    y, x0 = rnd(), rnd()
    for take in takes:
        x = ops.hmm_mix_fwd(y, x0, take, poison(float("nan")), B, S)
        want = torch.where(take.bool().repeat(B)[:, None], y, x0)
        assert torch.equal(x, want)
    # backward: a three-layer sequence (INIT at the top, add, the layer-0 form)
    dx2, dx1, dx0 = rnd(), rnd(), rnd()
    m2, m1 = (t.bool().repeat(B)[:, None] for t in takes[:2])
    zero = torch.zeros((), device=DEV)

    def run(pv):
        acc, dy2, dy1, out = poison(pv, torch.float32), poison(pv), poison(pv), poison(pv)
        r = ops.hmm_mix_bwd(dx2, takes[0], acc, B, S, dy=dy2, init=True)
        assert r is dy2
        acc_init = acc.clone()
        ops.hmm_mix_bwd(dx1, takes[1], acc, B, S, dy=dy1)
        acc_add = acc.clone()
        r = ops.hmm_mix_bwd(dx0, None, acc, B, S, dx0=out)
        assert r is out and torch.equal(acc, acc_add)          # the layer-0 form only reads the accumulator
        return acc_init, acc_add, dy2, dy1, out
    acc_init, acc_add, dy2, dy1, out = run(float("nan"))
    assert torch.equal(dy2, torch.where(m2, dx2, zero.to(dtype))) and torch.equal(dy1, torch.where(m1, dx1, zero.to(dtype)))
    assert not dy2[m2.expand_as(dy2).logical_not()].any()        # exact zeros, not small values
    want_init = torch.where(m2, zero, dx2.float())
    assert torch.equal(acc_init, want_init)
    assert not acc_init[m2.expand_as(acc_init)].any()            # rows no restarting row touches: exactly 0 after INIT
    want_add = want_init + torch.where(m1, zero, dx1.float())    # the same fp32 sums in the same order
    assert torch.equal(acc_add, want_add)
    assert torch.equal(out, (want_add + dx0.float()).to(dtype))
    again = run(-3.0)
    for a_, b_ in zip((acc_init, acc_add, dy2, dy1, out), again):
        assert torch.equal(a_.view(torch.int32 if a_.dtype == torch.float32 else torch.int16),
                           b_.view(torch.int32 if b_.dtype == torch.float32 else torch.int16))


def test_mix_wrappers_reject_bad_operands():
    from vct_amd import ops
    x = torch.zeros(6, 64, device=DEV)
    take = torch.zeros(3, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):
        ops.hmm_mix_fwd(x, x, take, torch.zeros(5, 64, device=DEV), 2, 3)         # rows != B * S
    with pytest.raises(ValueError):
        ops.hmm_mix_fwd(x, x, take.to(torch.int32), torch.zeros(6, 64, device=DEV), 2, 3)
    with pytest.raises(ValueError):
        ops.hmm_mix_bwd(x, take, torch.zeros(6, 64, device=DEV), 2, 3)            # neither dy nor dx0
    with pytest.raises(ValueError):
        ops.hmm_mix_bwd(x, take, torch.zeros(6, 64, device=DEV, dtype=torch.bfloat16), 2, 3, dy=torch.zeros_like(x))
    with pytest.raises(ValueError):
        ops.hmm_mix_fwd(torch.zeros(6, 66, device=DEV), torch.zeros(6, 66, device=DEV), take, torch.zeros(6, 66, device=DEV), 2, 3)   # VCT_E_ALIGN


# ---- reference parity --------------------------------------------------------------------------------------------------------
def _load(case, dtype):
    z = load_golden(f"hmm_{case}.npz")
    mc, V = model_config_of(z), int(z["vocab"])
    m = build_model(mc, V, DEV, dtype, hmm_params(mc, V, int(z["param_seed"])))
    n = len(mc["modal_shape"])
    return z, mc, m, [_dev(z[f"feats{i}"]) for i in range(n)], [_dev(z[f"mask{i}"]) for i in range(n)], _dev(z["ids"])


@pytest.mark.parametrize("dtype,tl,tg", [(torch.float32, 1e-4, 1e-3), (torch.bfloat16, 2e-2, 3e-2)])
@pytest.mark.parametrize("case", ["A", "B", "C", "D"])
def test_forward_backward_adam_vs_reference(case, dtype, tl, tg):
    z, mc, m, feats, masks, ids = _load(case, dtype)
    layers = mc["video_encoder"]["layer"]
    L, n, d = max(layers), len(layers), mc["embed_dim"]
    m.train()
    loss, _ = m._forward_loss(*m._video_inputs(feats, masks), ids, True)
    print(f"[hmm {case} {dtype}] loss {float(loss):.7f} ref {float(z['loss']):.7f}")
    assert abs(float(loss) - float(z["loss"])) < (1e-5 if dtype == torch.float32 else 2e-3) * float(z["loss"])
    enc_b = m.video_encoder._engine().cur
    shp = z["act/memory"].shape
    assert rel(enc_b.t["x0"].float().view(shp), z["act/layer_in0"]) < tl          # mm_src: layer 0 takes it as it is
    for l in range(L):
        e = rel(enc_b.t[f"L{l}.x"].float().view(shp), z[f"act/layer_in{l}"])
        print(f"[hmm {case} {dtype}] layer {l} input rel {e:.3e}")
        assert e < tl, l
    assert rel(enc_b.t["x_last"].float().view(shp), z["act/memory"]) < tl
    assert "nf.y" not in enc_b.t                                                    # no stack-final norm ran
    mem, gmask, agg = m.video_encoder(feats, masks)         # the module API: memory, the concatenated mask, agg_feats [B]
    assert rel(mem, z["act/memory"]) < tl
    assert np.array_equal(gmask.cpu().numpy(), z["act/gmask"])
    assert tuple(agg.shape) == (shp[0],) == z["act/agg"].shape
    firsts = np.cumsum([0] + [f.shape[1] + 1 for f in feats])[:-1].tolist()
    assert torch.equal(agg, torch.cat([mem[:, s] for s in firsts], dim=1).sum(dim=1))
    agg_err = float(np.linalg.norm(agg.detach().double().cpu().numpy() - z["act/agg"]))
    assert agg_err <= math.sqrt(n * d) * tl * float(np.linalg.norm(z["act/memory"])), agg_err      # (module docstring)
    opt = torch.optim.Adam(filter(lambda q: q.requires_grad, m.parameters()), lr=1e-4, betas=(0.9, 0.999))
    loss2 = m(feats, masks, ids)
    opt.zero_grad()
    loss2.backward()
    named = dict(m.named_parameters())
    tol = GradTol(f"hmm_{case}_vs_reference", dtype, tg)
    loose = GradTol(f"hmm_{case}_vs_reference_unify_weight_bf16_argmax", dtype, math.inf)
    moved = dtype == torch.bfloat16 and case == "B"
    gk = [k[len("grad/"):] for k in z.files if k.startswith("grad/")]
    assert sum(k.startswith("video_encoder.trans_enc_layers.") for k in gk) == 12 * L and not any("transformer_encoder" in k for k in gk)
    for k in gk:
        (loose if moved and ".unify." in k and k.endswith(".weight") else tol).add(k, rel(named[k].grad, z["grad/" + k]))
    if case == "B":
        head = z["grad_head/" + EMB]
        g = named[EMB].grad
        tol.add(EMB, rel(g[:len(head)], head))
        assert not g[len(head):].any()                     # rows nobody reads: exactly zero
        assert sorted(torch.nonzero(g.abs().sum(1)).flatten().tolist()) == z["emb_rows_read"].tolist()
    tol.report()
    if moved:
        loose.report()
    if dtype == torch.float32 and case == "B":
        p = {k: named[k].detach().cpu().numpy().astype(np.float64) for k in gk + [EMB]}
        opt.step()
        za = load_golden("hmm_B_adam.npz")
        for k in gk:
            upd_ref = za["adam1/" + k].astype(np.float64) - p[k]
            upd = named[k].detach().cpu().numpy().astype(np.float64) - p[k]
            big = np.abs(z["grad/" + k]) > 1e-5
            assert np.abs(upd - upd_ref)[big].max(initial=0) < 5e-6, k
        head = za["adam1_head/" + EMB].astype(np.float64)
        now = named[EMB].detach().cpu().numpy().astype(np.float64)
        big = np.abs(z["grad_head/" + EMB]) > 1e-5
        assert np.abs((now[:len(head)] - p[EMB][:len(head)]) - (head - p[EMB][:len(head)]))[big].max(initial=0) < 5e-6
        assert np.array_equal(now[len(head):], p[EMB][len(head):])


@pytest.mark.parametrize("B", [1, 3])
def test_case_B_greedy_ids_exact_fp32(B):
    z = load_golden("hmm_B.npz")
    zd = load_golden("hmm_B_decode.npz")
    mc, V = model_config_of(z), int(z["vocab"])
    m = build_model(mc, V, DEV, torch.float32, hmm_params(mc, V, int(zd["param_seed"])))
    f = [_dev(zd[f"b{B}/feats0"]), _dev(zd[f"b{B}/feats1"])]
    want = zd[f"b{B}/ys"]
    for masks in (None, [torch.zeros(B, 5, dtype=torch.bool, device=DEV), torch.zeros(B, 3, dtype=torch.bool, device=DEV)]):
        ys = m.greedy_decode_ids(f, masks, max_len=12)
        assert np.array_equal(ys.cpu().numpy()[:, :want.shape[1]], want)
        ys_ref = m.greedy_decode_ids(f, masks, max_len=12, kv_cache=False)
        assert torch.equal(ys, ys_ref)
    b1 = m.beam_decode_ids(f, None, beam_size=1, max_len=12)          # beam K = 1 is greedy
    g = m.greedy_decode_ids(f, None, max_len=12)
    for r in range(B):
        row = g[r].tolist()
        n = row.index(102) + 1 if 102 in row[1:] else len(row)
        assert b1[r].tolist()[:n] == row[:n]
    ys, maps = m.greedy_decode_ids(f, None, max_len=12, return_attn=True)
    assert torch.equal(ys, g) and tuple(maps.shape) == (B, 2, ys.shape[1] - 1, 10)
    assert float((maps.sum(-1) - 1).abs().max()) < 1e-3         # head-averaged softmax rows


# ---- executors ---------------------------------------------------------------------------------------------------------------
def test_every_executor_bitwise():
    """d 512, encoder [2, 1], 2 decoder layers, two streams with dropout on: eager = launch list = hipGraph."""
    from vct_amd.trainer import CaptionTrainer, FusedAdam
    mc = hmm_config([512, 128], [2, 1], d=512, H=8, ff=2048, dropout=0.1)
    f, k, ids = mm_batch(8, (6, 4), (512, 128), 9, 1000, seed=6, valid=[[6] * 8, [4, 3, 4, 2, 4, 4, 1, 4]])
    feats, masks, ids = [_dev(a) for a in f], [_dev(a) for a in k], _dev(ids)
    p = hmm_params(mc, 1000, 5)
    results = []
    for mode in ("eager", "list", "graph"):
        torch.manual_seed(11)          # the dropout seed tensor is drawn from torch's at construction
        m = build_model(mc, 1000, DEV, torch.bfloat16, p)
        m.train()
        opt = FusedAdam(m, lr=1e-4)
        tr = CaptionTrainer(m, opt, use_graph=(mode == "graph"), launch_list=(mode == "list"))
        losses = [tr.step(feats, masks, ids).clone() for _ in range(3)]
        torch.cuda.synchronize()
        if mode == "graph":
            assert tr.use_graph            # the step was really captured (no silent fall-back to eager)
        results.append((torch.cat(losses), m.flat_params.clone()))
        for n_ in ("video_encoder.trans_enc_layers.0.linear1.weight", "video_encoder.trans_enc_layers.1.norm2.bias",
                   "video_encoder.unify.1.weight", "video_encoder.modal_emb.modal_emb.weight"):
            assert not torch.equal(m._ps.params[n_].data.cpu(), torch.from_numpy(p[n_])), n_       # the optimizer stepped it
    assert torch.isfinite(results[0][0]).all()
    for lo, pa in results[1:]:
        assert torch.equal(lo, results[0][0]) and torch.equal(pa, results[0][1])


# ---- launch counts -----------------------------------------------------------------------------------------------------------
def test_mix_launch_counts(monkeypatch):
    from vct_amd import ops
    calls = []
    for name in ("hmm_mix_fwd", "hmm_mix_bwd"):
        orig = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _o=orig, _n=name, **k: (calls.append(_n), _o(*a, **k))[1])
    f, k, ids = mm_batch(3, (5, 3), [48, 24], 7, 131, seed=41, valid=[[5, 3, 4], [2, 3, 1]])
    feats, masks, ids = [_dev(a) for a in f], [_dev(a) for a in k], _dev(ids)

    def count(mc, params, decode=False):
        del calls[:]
        m = build_model(mc, 131, DEV, torch.float32, params)
        m.train()
        loss = m.train_step_kernels(feats, masks, ids)
        if decode:
            m.greedy_decode_ids(feats, None, max_len=4)
        assert torch.isfinite(loss).all()
        return calls.count("hmm_mix_fwd"), calls.count("hmm_mix_bwd")
    mc = encvar_config([48, 24])
    assert count(mc, encvar_params(mc, 131, 31), decode=True) == (0, 0)          # the default `mme` path never reaches them
    for layers, want in (([2, 2], (0, 0)), ([2, 1], (1, 2)), ([1, 3], (2, 3))):
        mc = hmm_config([48, 24], layers)
        assert count(mc, hmm_params(mc, 131, 31)) == want, layers


def test_equal_depths_without_norm_is_the_mme_stack_minus_its_final_norm():
    """hmme [2, 2] launches no mix: every layer's input is the previous output, so the memory equals the `mme` model's last layer
    output (its x_last, in front of the stack-final norm) on the same layer weights."""
    f, k, ids = mm_batch(3, (5, 3), [48, 24], 7, 131, seed=41, valid=[[5, 3, 4], [2, 3, 1]])
    feats, masks, ids = [_dev(a) for a in f], [_dev(a) for a in k], _dev(ids)
    mh = hmm_config([48, 24], [2, 2])
    ph = hmm_params(mh, 131, 31)
    pm = {k_.replace("trans_enc_layers.", "transformer_encoder.layers."): v for k_, v in ph.items()}
    pm["video_encoder.transformer_encoder.norm.weight"] = np.ones(64, np.float32)
    pm["video_encoder.transformer_encoder.norm.bias"] = np.zeros(64, np.float32)
    a = build_model(mh, 131, DEV, torch.float32, ph)
    b = build_model(encvar_config([48, 24]), 131, DEV, torch.float32, pm)
    a._forward_loss(feats, masks, ids, False)
    b._forward_loss(feats, masks, ids, False)
    xa, xb = a.video_encoder._engine().cur.t["x_last"], b.video_encoder._engine().cur.t["x_last"]
    assert rel(xa, xb) < 1e-6           # (fp32 rounding only: `mme` closes its last layer with the fused norm2 + final-norm launch)


# ---- resume, exchange --------------------------------------------------------------------------------------------------------
def _small_bf16(seed):
    torch.manual_seed(seed)
    m = build_model(hmm_config([48, 24], [2, 1], dropout=0.1), 131, DEV, torch.bfloat16)
    m.train()
    return m


def _small_batch(k):
    f, mk, ids = mm_batch(6, (5, 3), [48, 24], 9, 131, seed=70 + k, valid=[[5, 3, 4, 5, 2, 5], [2, 3, 1, 3, 3, 2]])
    return [_dev(a) for a in f], [_dev(a) for a in mk], _dev(ids)


def test_resume_is_bit_exact(tmp_path):
    """2 steps + save + load into a fresh model / optimizer + 1 step == 3 uninterrupted steps, dropout active."""
    from vct_amd import checkpoint as ck
    from vct_amd.trainer import CaptionTrainer, FusedAdam

    def fresh(seed):
        m = _small_bf16(seed)
        opt = FusedAdam(m, lr=1e-3)
        return m, opt, CaptionTrainer(m, opt)
    mA, optA, trA = fresh(11)
    lossA = torch.cat([trA.step(*_small_batch(k)).clone() for k in range(3)])
    mB, optB, trB = fresh(11)
    lossB = torch.cat([trB.step(*_small_batch(k)).clone() for k in range(2)])
    ck.save_training_state(str(tmp_path / "s.pt"), mB, optB, epoch=0)
    mC, optC, trC = fresh(99)               # different init: everything must come from the file
    ck.load_training_state(str(tmp_path / "s.pt"), mC, optC)
    assert torch.equal(mC.flat_params, mB.flat_params)
    lossC = trC.step(*_small_batch(2)).clone()
    torch.cuda.synchronize()
    assert torch.equal(torch.cat([lossB, lossC]), lossA)
    assert torch.equal(mC.flat_params, mA.flat_params)
    assert torch.equal(optC.exp_avg_sq, optA.exp_avg_sq) and int(optC.step_dev) == int(optA.step_dev) == 3


def test_exchange_path_world1_step_is_the_plain_step():
    from vct_amd.comm import RcclColl
    from vct_amd.trainer import CaptionTrainer, FusedAdam, ShardedExchange
    m0 = _small_bf16(11)
    m0._seed.fill_(1234)
    tr0 = CaptionTrainer(m0, FusedAdam(m0, lr=1e-3))
    l0 = tr0.step(*_small_batch(0)).clone()
    m = _small_bf16(11)
    m._seed.fill_(1234)
    opt = FusedAdam(m, lr=1e-3)
    coll = RcclColl(device=torch.device("cuda", 0))
    assert coll.world == 1
    tr = CaptionTrainer(m, opt, ShardedExchange(m, opt, coll, sharded=True))
    l1 = tr.step(*_small_batch(0)).clone()
    torch.cuda.synchronize()
    assert torch.equal(l0, l1) and torch.equal(m.flat_params, m0.flat_params)
    assert not torch.equal(m.flat_params, _small_bf16(11).flat_params)          # (the step moved the parameters)
    coll.close()
