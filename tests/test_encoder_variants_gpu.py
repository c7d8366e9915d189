"""The encoder's options on the GPU (temporal 'embedding', aggregation 'max', do_norm): the vct_enc_frontend_ex_* kernels against an
fp64 restatement on the same inputs, dropout behind the norm, parity with the reference's MultiModalEncoder
(tests/golden/encvar_*.npz, tools/make_golden_encoder_variants.py), decode, the three executors, and that the shipped combination
never reaches the new kernels.

Tolerances: kernels as test_multimodal_gpu.test_frontend_kernels_vs_fp64 (1e-5 fp32, 1e-2 bf16, 1e-4 for the fp32 parameter
gradients); parity as tests/test_multimodal_gpu.py (fp32 loss 1e-5 rel, activations 1e-4, gradients 1e-3; bf16 activations 2e-2,
loss 2e-3, gradients 3e-2 through helpers.GradTol).  bf16 with 'max': rounding the unify output to bf16 can move a near-tied maximum
to another row, which changes unify.*.weight gradients only (everything else sums over the rows); their error against the fp32
reference goes to the tolerance log through a GradTol with an infinite bound and is not asserted -- the fp32 parity and the kernel
test carry them."""
import itertools
import math

import numpy as np
import pytest
import torch

from encvar_ref import encvar_config, encvar_params, temporal_index
from helpers import GradTol, build_model, load_golden, model_config_of, rel
from mm_ref import mm_batch
from test_multimodal_gpu import _Paths

pytestmark = pytest.mark.gpu
DEV = "cuda"
EMB = "video_encoder.temp_emb.embedding.weight"
SITE = 998


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(t):
    return t.double().cpu().numpy()


# ---- kernels ---------------------------------------------------------------------------------------------------------------
class _Case:
    """Random operands of one front-end call (the same, dtype-rounded, values go to the kernels and to the fp64 restatement)."""

    def __init__(self, dtype, Ts, B, d, seed=0, ties=False):
        g = torch.Generator(device="cpu").manual_seed(seed)
        self.dtype, self.Ts, self.B, self.d, self.n = dtype, Ts, B, d, len(Ts)
        n, S = self.n, sum(t + 1 for t in Ts)
        self.S = S
        us = [torch.randn(B, t, d, generator=g) for t in Ts]
        if ties:        # exact ties at the column maximum: two rows (the first two), two TRAILING rows, three rows
            for u, t in zip(us, Ts):
                if t >= 2:
                    u[:, 0, 0] = u[:, 1, 0] = 7.0
                    u[:, t - 1, 1] = u[:, t - 2, 1] = 6.0
                if t >= 3:
                    u[:, 0, 2] = u[:, 1, 2] = u[:, t - 1, 2] = 5.0
                    u[:, 1, 3] = u[:, t - 1, 3] = 4.0
        self.us = [u.reshape(B * t, d).to(DEV).to(dtype).contiguous() for u, t in zip(us, Ts)]
        self.masks = [(torch.rand(B, t, generator=g) < 0.4).to(DEV) for t in Ts]
        self.temp = torch.randn(S, d, generator=g).to(DEV)
        self.emb_w = torch.randn(512, d, generator=g).to(DEV)
        self.tidx_np = temporal_index(Ts)
        self.tidx = torch.from_numpy(self.tidx_np.astype(np.int32)).to(DEV)
        self.modal = torch.randn(2 * n, d, generator=g).to(DEV) if n > 1 else None
        labels = []
        for i, t in enumerate(Ts):
            labels += [i + n] + [i] * t
        self.labels_np = np.array(labels)
        self.labels = torch.tensor(labels, dtype=torch.int32, device=DEV) if n > 1 else None
        self.gamma = (1.0 + 0.1 * torch.randn(d, generator=g)).to(DEV)
        self.beta = (0.1 * torch.randn(d, generator=g)).to(DEV)
        self.dx = torch.randn(B * S, d, generator=g).to(DEV).to(dtype)
        self.seed = torch.tensor([12345], dtype=torch.int32, device=DEV)

    def kw(self, agg, learned, norm, p=None):
        kw = dict(agg=agg, modal_w=self.modal, labels=self.labels)
        if learned:
            kw.update(tidx=self.tidx, emb_w=self.emb_w)
        else:
            kw.update(temp=self.temp)
        if norm:
            mean, rstd = (torch.full((self.B * self.S,), float("nan"), device=DEV) for _ in range(2))
            kw["norm"] = dict(gamma=self.gamma, beta=self.beta, mean=mean, rstd=rstd, dropout=None if p is None else (self.seed, SITE, p))
        return kw

    # fp64 restatement of MMEncoder.py:244-273 on the stored operands
    def ref_pre(self, agg, learned):
        B, d = self.B, self.d
        pre = np.zeros((B, self.S, d))
        arg, at = [], 0
        for i, t in enumerate(self.Ts):
            u = _np(self.us[i]).reshape(B, t, d)
            pre[:, at] = u.max(1) if agg == "max" else u.mean(1)
            arg.append(u.argmax(1))           # first occurrence, like torch's max-pool backward
            pre[:, at + 1:at + 1 + t] = u
            at += t + 1
        add = _np(self.emb_w)[self.tidx_np] if learned else _np(self.temp)
        if self.n > 1:
            add = add + _np(self.modal)[self.labels_np]
        return pre + add[None], arg

    def ref_norm(self, pre):
        mean = pre.mean(-1, keepdims=True)
        rstd = 1.0 / np.sqrt(pre.var(-1, keepdims=True) + 1e-5)
        xh = (pre - mean) * rstd
        return xh * _np(self.gamma) + _np(self.beta), xh, rstd

    def ref_bwd(self, g, agg, learned, norm, arg, xh=None, rstd=None):
        """g [B, S, d]: the gradient of the norm's output (mask and scale applied), or of pre without the norm."""
        B, d = self.B, self.d
        out = {}
        if norm:
            gg = g * _np(self.gamma)
            dpre = rstd * (gg - gg.mean(-1, keepdims=True) - xh * (gg * xh).mean(-1, keepdims=True))
            out["dgamma"], out["dbeta"] = (g * xh).sum((0, 1)), g.sum((0, 1))
        else:
            dpre = g
        out["du"], at = [], 0
        for i, t in enumerate(self.Ts):
            du = dpre[:, at + 1:at + 1 + t].copy()
            if agg == "max":
                for b in range(B):
                    du[b, arg[i][b], np.arange(d)] += dpre[b, at]
            else:
                du += dpre[:, at:at + 1] / t
            out["du"].append(du)
            at += t + 1
        if self.n > 1:
            out["d_modal"] = np.zeros((2 * self.n, d))
            for s, l in enumerate(self.labels_np):
                out["d_modal"][l] += dpre[:, s].sum(0)
        if learned:
            out["d_emb"] = np.zeros((512, d))
            for s, e in enumerate(self.tidx_np):
                out["d_emb"][e] += dpre[:, s].sum(0)
        return out

    def run_bwd(self, agg, learned, norm, kw, poison):
        from vct_amd import ops
        B, d, n = self.B, self.d, self.n
        dus = [torch.full((B * t, d), poison, device=DEV).to(self.dtype) for t in self.Ts]
        d_modal = torch.full((2 * n, d), poison, device=DEV) if n > 1 else None
        d_emb = torch.full((512, d), poison, device=DEV) if learned else None
        dpre = torch.full((B * self.S, d), poison, device=DEV) if norm else None
        ws = torch.full((B * n * 2 * d,), poison, device=DEV) if norm else None
        ops.enc_frontend_ex_bwd(self.dx, dus, B, self.Ts, us=self.us, d_modal=d_modal, d_emb=d_emb, dpre=dpre, param_ws=ws, **kw)
        return dus, d_modal, d_emb, ws


def _close(got, want, tol):
    return np.abs(got - want).max() < tol * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("Ts,B,d", [((1,), 1, 64), ((3,), 2, 64), ((3, 2), 3, 64), ((4, 1, 2), 2, 64), ((5, 3, 2, 1), 4, 64),
                                    ((3, 2), 3, 72)])
def test_ex_kernels_vs_fp64(dtype, Ts, B, d):
    from vct_amd import ops
    c = _Case(dtype, Ts, B, d, seed=len(Ts) + B, ties=True)
    S, n = c.S, c.n
    tol = 1e-5 if dtype == torch.float32 else 1e-2
    for agg, learned, norm in itertools.product(("avg", "max"), (False, True), (False, True)):
        what = (agg, learned, norm)
        kw = c.kw(agg, learned, norm)
        x0 = torch.full((B * S, d), float("nan"), device=DEV).to(dtype)
        kp = torch.full((B, S), 7, dtype=torch.uint8, device=DEV)
        ops.enc_frontend_ex_fwd(c.us, [m.view(torch.uint8) for m in c.masks], x0, kp, B, Ts, **kw)
        pre, arg = c.ref_pre(agg, learned)
        want, xh, rstd = c.ref_norm(pre) if norm else (pre, None, None)
        assert _close(_np(x0).reshape(B, S, d), want, tol), what
        want_kp, at = np.zeros((B, S), np.uint8), 0
        for i, t in enumerate(Ts):
            want_kp[:, at + 1:at + 1 + t] = c.masks[i].cpu().numpy()
            at += t + 1
        assert np.array_equal(kp.cpu().numpy(), want_kp), what
        if norm:
            assert _close(_np(kw["norm"]["mean"]), pre.mean(-1).reshape(-1), 1e-5) and _close(_np(kw["norm"]["rstd"]), rstd.reshape(-1), 1e-4), what
        # backward: every output starts as NaN, the whole [512, d] embedding gradient included
        wb = c.ref_bwd(_np(c.dx).reshape(B, S, d), agg, learned, norm, arg, xh, rstd)
        dus, d_modal, d_emb, ws = c.run_bwd(agg, learned, norm, kw, float("nan"))
        for i, t in enumerate(Ts):
            assert _close(_np(dus[i]).reshape(B, t, d), wb["du"][i], tol), (what, i)
        if n > 1:
            assert _close(_np(d_modal), wb["d_modal"], 1e-4), what
        if learned:
            assert _close(_np(d_emb), wb["d_emb"], 1e-4), what
            unread = np.setdiff1d(np.arange(512), c.tidx_np)
            assert torch.equal(d_emb[_dev(unread)], torch.zeros(len(unread), d, device=DEV)), what      # exactly 0, not "small"
        if norm:
            part = _np(ws).reshape(B * n, 2, d).sum(0)
            assert _close(part[0], wb["dgamma"], 1e-4) and _close(part[1], wb["dbeta"], 1e-4), what
        if agg == "max" and not norm:
            # the tie columns: the whole gradient of the aggregation row on the FIRST maximal row, the later ones get their own row only
            g = c.dx.view(B, S, d)
            at = 0
            for i, t in enumerate(Ts):
                du = dus[i].view(B, t, d)
                if t >= 2:
                    assert torch.equal(du[:, 1, 0], g[:, at + 2, 0]) and torch.equal(du[:, t - 1, 1], g[:, at + t, 1]), (what, i)
                    first = (g[:, at + 1, 0].float() + g[:, at, 0].float()).to(dtype)
                    assert torch.equal(du[:, 0, 0], first), (what, i)
                    trailing = (g[:, at + t - 1, 1].float() + g[:, at, 1].float()).to(dtype)
                    assert torch.equal(du[:, t - 2, 1], trailing), (what, i)
                if t >= 3:
                    assert torch.equal(du[:, 1, 2], g[:, at + 2, 2]) and torch.equal(du[:, t - 1, 2], g[:, at + t, 2]), (what, i)
                at += t + 1
        # fixed reduction order: a second run into differently poisoned buffers is bitwise the same
        dus2, d_modal2, d_emb2, ws2 = c.run_bwd(agg, learned, norm, kw, -3.0)
        for a_, b_ in zip(dus + [d_modal, d_emb, ws], dus2 + [d_modal2, d_emb2, ws2]):
            assert (a_ is None and b_ is None) or torch.equal(a_, b_), what


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_dropout_behind_the_norm(dtype):
    """x0 = Dropout(LayerNorm(pre)) (MMEncoder.py:273): the mask falls on the norm's OUTPUT, and the backward re-applies it to dx."""
    from vct_amd import ops
    B, Ts, d = 8, (10, 6), 64
    c = _Case(dtype, Ts, B, d, seed=3)
    S, n = c.S, c.n
    masks = [m.view(torch.uint8) for m in c.masks]

    def fwd(p):
        kw = c.kw("max", True, True, p=p)
        x0 = torch.full((B * S, d), float("nan"), device=DEV).to(dtype)
        ops.enc_frontend_ex_fwd(c.us, masks, x0, None, B, Ts, **kw)
        return x0, kw
    y0, kw0 = fwd(0.0)
    kw_plain = c.kw("max", True, True)
    x_plain = torch.full((B * S, d), float("nan"), device=DEV).to(dtype)
    ops.enc_frontend_ex_fwd(c.us, masks, x_plain, None, B, Ts, **kw_plain)
    assert torch.equal(y0, x_plain)                       # p = 0 with a seed: the norm-only result, bitwise
    y, kw = fwd(0.5)
    assert y.numel() >= 8000
    kept = y != 0
    assert torch.equal(y[kept], (y0 * 2)[kept])           # every element: 0, or the undropped value x 1 / (1 - p)
    live = y0 != 0
    frac = float((kept & live).sum()) / float(live.sum())
    assert abs(frac - 0.5) < 0.05, frac
    # backward = the fp64 LayerNorm backward of dx x mask x 2, the mask read off the forward output
    pre, arg = c.ref_pre("max", True)
    _, xh, rstd = c.ref_norm(pre)
    g = _np(c.dx).reshape(B, S, d) * (kept.cpu().numpy().reshape(B, S, d) * 2.0)
    wb = c.ref_bwd(g, "max", True, True, arg, xh, rstd)
    dus, d_modal, d_emb, ws = c.run_bwd("max", True, True, kw, float("nan"))
    tol = 1e-5 if dtype == torch.float32 else 1e-2
    for i, t in enumerate(Ts):
        assert _close(_np(dus[i]).reshape(B, t, d), wb["du"][i], tol), i
    part = _np(ws).reshape(B * n, 2, d).sum(0)
    assert _close(_np(d_modal), wb["d_modal"], 1e-4) and _close(_np(d_emb), wb["d_emb"], 1e-4)
    assert _close(part[0], wb["dgamma"], 1e-4) and _close(part[1], wb["dbeta"], 1e-4)
    # p = 0 in the backward too
    a, b = c.run_bwd("max", True, True, kw0, float("nan")), c.run_bwd("max", True, True, kw_plain, float("nan"))
    assert all(torch.equal(x, z) for x, z in zip(a[0] + list(a[1:]), b[0] + list(b[1:])))


# ---- the shipped path stays where it is -------------------------------------------------------------------------------------
def test_shipped_combination_through_the_new_entry_point_equals_mm_frontend_bitwise():
    from vct_amd import ops
    for dtype in (torch.float32, torch.bfloat16):
        c = _Case(dtype, (3, 2), 2, 64, seed=9)
        masks = [m.view(torch.uint8) for m in c.masks]
        x_new = torch.full((2 * c.S, 64), float("nan"), device=DEV).to(dtype)
        kp_new = torch.full((2, c.S), 7, dtype=torch.uint8, device=DEV)
        ops.enc_frontend_ex_fwd(c.us, masks, x_new, kp_new, 2, c.Ts, **c.kw("avg", False, False))
        x_old = torch.full((2 * c.S, 64), float("nan"), device=DEV).to(dtype)
        kp_old = torch.full((2, c.S), 7, dtype=torch.uint8, device=DEV)
        ops.mm_frontend_fwd(c.us, masks, c.temp, c.modal, c.labels, x_old, kp_old, 2, c.Ts)
        assert torch.equal(x_new, x_old) and torch.equal(kp_new, kp_old)


@pytest.mark.parametrize("shapes,Ts", [([48], (5,)), ([48, 24], (5, 3))])
def test_default_config_never_calls_the_new_wrappers(monkeypatch, shapes, Ts):
    from vct_amd import ops
    calls = []
    for name in ("enc_frontend_ex_fwd", "enc_frontend_ex_bwd"):
        orig = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _o=orig, _n=name, **k: (calls.append(_n), _o(*a, **k))[1])
    mc = encvar_config(shapes)
    m = build_model(mc, 131, DEV, torch.float32, encvar_params(mc, 131, 31))
    m.train()
    f, k, ids = mm_batch(3, Ts, shapes, 7, 131, seed=41, valid=[[5, 3, 4], [2, 3, 1]][:len(Ts)])
    loss = m.train_step_kernels([_dev(a) for a in f], [_dev(a) for a in k], _dev(ids))
    m.greedy_decode_ids([_dev(a) for a in f], None, max_len=4)
    assert torch.isfinite(loss).all() and calls == []
    # ... and a variant does (the spy works)
    mc = encvar_config(shapes, "max")
    m = build_model(mc, 131, DEV, torch.float32, encvar_params(mc, 131, 31))
    m.train()
    m.train_step_kernels([_dev(a) for a in f], [_dev(a) for a in k], _dev(ids))
    assert calls == ["enc_frontend_ex_fwd", "enc_frontend_ex_bwd"]


# ---- reference parity --------------------------------------------------------------------------------------------------------
def _load(case, dtype):
    z = load_golden(f"encvar_{case}.npz")
    mc, V = model_config_of(z), int(z["vocab"])
    m = build_model(mc, V, DEV, dtype, encvar_params(mc, V, int(z["param_seed"])))
    n = len(mc["modal_shape"])
    return z, m, [_dev(z[f"feats{i}"]) for i in range(n)], [_dev(z[f"mask{i}"]) for i in range(n)], _dev(z["ids"])


@pytest.mark.parametrize("dtype,tl,tg", [(torch.float32, 1e-4, 1e-3), (torch.bfloat16, 2e-2, 3e-2)])
@pytest.mark.parametrize("case", ["E", "M", "N", "X", "S"])      # S: one stream on the FIXED table ("max" + do_norm; front-end gradients only)
def test_forward_backward_adam_vs_reference(case, dtype, tl, tg):
    z, m, feats, masks, ids = _load(case, dtype)
    m.train()
    loss, _ = m._forward_loss(*m._video_inputs(feats, masks), ids, True)
    assert abs(float(loss) - float(z["loss"])) < (1e-5 if dtype == torch.float32 else 2e-3) * float(z["loss"])
    enc_b = m.video_encoder._engine().cur
    assert rel(enc_b.t["x0"].float().view(z["act/mm_src"].shape), z["act/mm_src"]) < tl
    assert rel(enc_b.t["nf.y"].float().view(z["act/memory"].shape), z["act/memory"]) < tl
    mem, gmask, agg = m.video_encoder(feats, masks)         # the module API: memory, the concatenated mask, the agg row
    assert rel(mem, z["act/memory"]) < tl and rel(agg, z["act/agg"]) < tl
    assert np.array_equal(gmask.cpu().numpy(), z["act/gmask"])
    opt = torch.optim.Adam(filter(lambda q: q.requires_grad, m.parameters()), lr=1e-4, betas=(0.9, 0.999))
    loss2 = m(feats, masks, ids)
    opt.zero_grad()
    loss2.backward()
    named = dict(m.named_parameters())
    tol = GradTol(f"encvar_{case}_vs_reference", dtype, tg)
    # bf16 + 'max': a near-tied maximum may sit on another row after rounding -- unify.*.weight gradients are logged, not asserted
    loose = GradTol(f"encvar_{case}_vs_reference_unify_weight_bf16_argmax", dtype, math.inf)
    moved = dtype == torch.bfloat16 and case in ("M", "X", "S")
    gk = [k[len("grad/"):] for k in z.files if k.startswith("grad/")]
    want_new = {"E": [EMB], "M": [], "N": ["video_encoder.norm.weight", "video_encoder.norm.bias"],
                "X": [EMB, "video_encoder.norm.weight", "video_encoder.norm.bias"],
                "S": ["video_encoder.norm.weight", "video_encoder.norm.bias"]}[case]
    assert all(k in gk or k == EMB for k in want_new)
    for k in gk:
        (loose if moved and ".unify." in k and k.endswith(".weight") else tol).add(k, rel(named[k].grad, z["grad/" + k]))
    if EMB in want_new:
        head = z["grad_head/" + EMB]
        g = named[EMB].grad
        tol.add(EMB, rel(g[:len(head)], head))
        assert not g[len(head):].any()                     # rows nobody reads: exactly zero
        assert sorted(torch.nonzero(g.abs().sum(1)).flatten().tolist()) == z["emb_rows_read"].tolist()
    tol.report()
    if moved:
        loose.report()
    if dtype == torch.float32 and case == "X":
        p = {k: named[k].detach().cpu().numpy().astype(np.float64) for k in gk + [EMB]}
        opt.step()
        za = load_golden("encvar_X_adam.npz")
        for k in gk:
            upd_ref = za["adam1/" + k].astype(np.float64) - p[k]
            upd = named[k].detach().cpu().numpy().astype(np.float64) - p[k]
            big = np.abs(z["grad/" + k]) > 1e-5
            assert np.abs(upd - upd_ref)[big].max(initial=0) < 5e-6, k
        head = za["adam1_head/" + EMB].astype(np.float64)
        now = named[EMB].detach().cpu().numpy().astype(np.float64)
        big = np.abs(z["grad_head/" + EMB]) > 1e-5
        assert np.abs((now[:len(head)] - p[EMB][:len(head)]) - (head - p[EMB][:len(head)]))[big].max(initial=0) < 5e-6
        assert np.array_equal(now[len(head):], p[EMB][len(head):])          # zero gradient, zero moments: the row does not move


@pytest.mark.parametrize("B", [1, 3])
def test_case_X_greedy_ids_exact_fp32(B):
    z = load_golden("encvar_X.npz")
    zd = load_golden("encvar_X_decode.npz")
    mc, V = model_config_of(z), int(z["vocab"])
    m = build_model(mc, V, DEV, torch.float32, encvar_params(mc, V, int(zd["param_seed"])))
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


# ---- executors ---------------------------------------------------------------------------------------------------------------
def test_all_options_on_every_executor_bitwise():
    """d 512, 2 + 2 layers, two streams, 'embedding' + 'max' + do_norm with dropout on: eager = launch list = hipGraph, and both stacks
    still run sample-stationary behind the new front end (S = 12)."""
    from vct_amd.trainer import CaptionTrainer, FusedAdam
    mc = encvar_config([512, 128], "max", "embedding", True, d=512, H=8, ff=2048, dropout=0.1)
    f, k, ids = mm_batch(8, (6, 4), (512, 128), 9, 1000, seed=6, valid=[[6] * 8, [4, 3, 4, 2, 4, 4, 1, 4]])
    feats, masks, ids = [_dev(a) for a in f], [_dev(a) for a in k], _dev(ids)
    p = encvar_params(mc, 1000, 5)
    results = []
    for mode in ("eager", "list", "graph"):
        torch.manual_seed(11)          # the dropout seed tensor is drawn from torch's at construction
        m = build_model(mc, 1000, DEV, torch.bfloat16, p)
        m.train()
        if mode == "eager":
            with _Paths() as pth:
                m.train_step_kernels(feats, masks, ids)
            assert sorted(pth.seen) == ["DecoderEngine", "EncoderEngine"]
            torch.manual_seed(11)
            m = build_model(mc, 1000, DEV, torch.bfloat16, p)
            m.train()
        opt = FusedAdam(m, lr=1e-4)
        tr = CaptionTrainer(m, opt, use_graph=(mode == "graph"), launch_list=(mode == "list"))
        losses = [tr.step(feats, masks, ids).clone() for _ in range(3)]
        torch.cuda.synchronize()
        if mode == "graph":
            assert tr.use_graph            # the step was really captured (no silent fall-back to eager)
        results.append((torch.cat(losses), m.flat_params.clone()))
        for n_ in (EMB, "video_encoder.norm.weight", "video_encoder.norm.bias"):
            assert not torch.equal(m._ps.params[n_].data.cpu(), torch.from_numpy(p[n_])), n_       # the optimizer stepped it
    assert torch.isfinite(results[0][0]).all()
    for lo, pa in results[1:]:
        assert torch.equal(lo, results[0][0]) and torch.equal(pa, results[0][1])
