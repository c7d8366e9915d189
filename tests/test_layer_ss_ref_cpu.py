"""The fp64 reference of the sample-stationary stack kernels (tests/layer_ss_ref.py) checked before it is trusted: its layer functions
against torch.nn's post-norm Transformer layers (forward values and input gradients to 1e-10), its prologues against the oracle's front
end and embedding, its stream-order tables against the block lists the engine packs (engine/stack.py: _ss_stream, _ss_stream_bwd), and
the conventions torch does not have (zero output of a fully masked row, the pair hash of the dropout counters)."""
import numpy as np
import pytest
import torch

import layer_ss_ref as R
import vct_oracle as O

D, NH = 512, 8
F64 = torch.float64


def close(what, got, ref, tol=1e-10):
    err = float((got - ref).abs().max() / ref.abs().max())
    assert err < tol, (what, err)


def _perturb_norms(mod, g):
    with torch.no_grad():
        for n, p in mod.named_parameters():
            if "norm" in n:
                p.add_(0.1 * torch.randn(p.shape, generator=g, dtype=F64))
            elif n.endswith("bias"):
                p.copy_(0.1 * torch.randn(p.shape, generator=g, dtype=F64))


def _weights_of(m, cross):
    w = dict(w_in=m.self_attn.in_proj_weight, b_in=m.self_attn.in_proj_bias, w_o=m.self_attn.out_proj.weight, b_o=m.self_attn.out_proj.bias,
             w1=m.linear1.weight, b1=m.linear1.bias, w2=m.linear2.weight, b2=m.linear2.bias, n1=(m.norm1.weight, m.norm1.bias))
    if cross:
        w.update(c_in=m.multihead_attn.in_proj_weight, cb_in=m.multihead_attn.in_proj_bias, c_o=m.multihead_attn.out_proj.weight,
                 cb_o=m.multihead_attn.out_proj.bias, n2=(m.norm2.weight, m.norm2.bias), n3=(m.norm3.weight, m.norm3.bias))
    else:
        w["n3"] = (m.norm2.weight, m.norm2.bias)
    return {k: (tuple(t.detach() for t in v) if isinstance(v, tuple) else v.detach()) for k, v in w.items()}


def _masks(B, L, causal):
    kpm = torch.zeros(B, L, dtype=torch.bool)
    kpm[0, L - 2:] = True
    kpm[B - 1, 1:] = True                       # only key 0 left
    att = torch.triu(torch.ones(L, L, dtype=torch.bool), 1) if causal else None
    return kpm, att


@pytest.mark.parametrize("act", ["gelu", "relu"])
@pytest.mark.parametrize("causal", [False, True])
def test_encoder_layer_equals_torch(act, causal):
    B, L, ff = 3, 7, 512
    g = torch.Generator().manual_seed(1)
    m = torch.nn.TransformerEncoderLayer(D, NH, ff, dropout=0.0, activation=act, batch_first=True, norm_first=False).double().train()
    _perturb_norms(m, g)
    x = torch.randn(B, L, D, generator=g, dtype=F64, requires_grad=True)
    dy = torch.randn(B * L, D, generator=g, dtype=F64)
    kpm, att = _masks(B, L, causal)
    y = m(x, src_mask=att, src_key_padding_mask=kpm).reshape(B * L, D)
    y.backward(dy)
    w = _weights_of(m, False)
    c = R.Cfg(B, L, ff, act, causal=causal, kpm=kpm)
    out, _ = R.layer_fwd(x.detach().reshape(B * L, D), w, c, (0,) * 6)
    close("encoder layer output", out["n3.y"], y.detach())
    sv = dict(x=x.detach().reshape(B * L, D), qkv=out["qkv"], a=out["a"], x1=out["n1.y"], hpre=out["hpre"], f=out["f"])
    sv.update({k: out[k] for k in ("n1.mean", "n1.rstd", "n3.mean", "n3.rstd")})
    r = R.layer_bwd(dy, sv, w, c, (0,) * 4)
    close("encoder layer input gradient", r["dx"], x.grad.reshape(B * L, D))
    # the partial rows summed over the samples are the LayerNorm parameter gradients
    close("norm2 dgamma", r["n3.ws"][:, 0].sum(0), m.norm2.weight.grad)
    close("norm2 dbeta", r["n3.ws"][:, 1].sum(0), m.norm2.bias.grad)
    close("norm1 dgamma", r["n1.ws"][:, 0].sum(0), m.norm1.weight.grad)
    close("norm1 dbeta", r["n1.ws"][:, 1].sum(0), m.norm1.bias.grad)
    # the gradients the weight-gradient products read: dW = d(out)^T in
    close("linear2 dW", r["df"].t() @ out["h"], m.linear2.weight.grad)
    close("linear1 dW", r["dhpre"].t() @ out["n1.y"], m.linear1.weight.grad)
    close("out_proj dW", r["da"].t() @ out["o"], m.self_attn.out_proj.weight.grad)
    close("in_proj dW", r["dqkv"].t() @ x.detach().reshape(B * L, D), m.self_attn.in_proj_weight.grad)


@pytest.mark.parametrize("act", ["gelu", "relu"])
def test_decoder_layer_equals_torch(act):
    B, L, Lm, ff = 3, 6, 5, 512
    g = torch.Generator().manual_seed(2)
    m = torch.nn.TransformerDecoderLayer(D, NH, ff, dropout=0.0, activation=act, batch_first=True, norm_first=False).double().train()
    _perturb_norms(m, g)
    x = torch.randn(B, L, D, generator=g, dtype=F64, requires_grad=True)
    mem = torch.randn(B, Lm, D, generator=g, dtype=F64, requires_grad=True)
    dy = torch.randn(B * L, D, generator=g, dtype=F64)
    kpm, att = _masks(B, L, True)
    y = m(x, mem, tgt_mask=att, tgt_key_padding_mask=kpm).reshape(B * L, D)
    y.backward(dy)
    x2, mem2 = (t.detach().clone().requires_grad_(True) for t in (x, mem))
    c = R.Cfg(B, L, ff, act, Lm=Lm, mem=mem2.reshape(B * Lm, D), causal=True, kpm=kpm)
    out, _ = R.layer_fwd(x2.reshape(B * L, D), _weights_of(m, True), c, (0,) * 6)
    close("decoder layer output", out["n3.y"].detach(), y.detach())
    out["n3.y"].backward(dy)
    close("decoder layer input gradient", x2.grad, x.grad)
    close("decoder layer memory gradient", mem2.grad, mem.grad)


def test_final_norm_and_stack_equal_torch():
    B, L, ff = 2, 5, 512
    g = torch.Generator().manual_seed(3)
    layer = torch.nn.TransformerEncoderLayer(D, NH, ff, dropout=0.0, activation="gelu", batch_first=True).double()
    enc = torch.nn.TransformerEncoder(layer, 3, norm=torch.nn.LayerNorm(D).double(), enable_nested_tensor=False).train()
    with torch.no_grad():
        for l in enc.layers:                    # (the clones share one initialisation: give every layer its own weights)
            for p in l.parameters():
                if p.dim() == 2:
                    p.copy_(0.05 * torch.randn(p.shape, generator=g, dtype=F64))
    _perturb_norms(enc, g)
    x = torch.randn(B, L, D, generator=g, dtype=F64, requires_grad=True)
    dy = torch.randn(B * L, D, generator=g, dtype=F64)
    y = enc(x).reshape(B * L, D)
    y.backward(dy)
    ws = [_weights_of(l, False) for l in enc.layers]
    c = R.Cfg(B, L, ff)
    final = (enc.norm.weight.detach(), enc.norm.bias.detach())
    res = R.stack_fwd(x.detach().reshape(B * L, D), ws, c, [(0,) * 6] * 3, final=final)
    close("stack output", res[-1][0]["nf.y"], y.detach())
    saved, xin = [], x.detach().reshape(B * L, D)
    for out, _ in res:
        sv = dict(x=xin, qkv=out["qkv"], a=out["a"], x1=out["n1.y"], hpre=out["hpre"], f=out["f"])
        sv.update({k: out[k] for k in ("n1.mean", "n1.rstd", "n3.mean", "n3.rstd")})
        saved.append(sv)
        xin = out["n3.y"]
    last = res[-1][0]
    r, nf_ws = R.stack_bwd(dy, saved, ws, c, [(0,) * 4] * 3, final=final[0], y_last=last["n3.y"], nf_stats=(last["nf.mean"], last["nf.rstd"]))
    close("stack input gradient", r[0]["dx"], x.grad.reshape(B * L, D))
    close("final norm dgamma", nf_ws[:, 0].sum(0), enc.norm.weight.grad)
    close("final norm dbeta", nf_ws[:, 1].sum(0), enc.norm.bias.grad)


def test_fully_masked_row_is_zero_and_dropout_scales():
    B, L = 2, 4
    g = torch.Generator().manual_seed(4)
    q, k, v = (torch.randn(B * L, D, generator=g, dtype=F64) for _ in range(3))
    kpm = torch.zeros(B, L, dtype=torch.bool)
    kpm[1] = True
    o = R.attention(q, k, v, B, L, L, False, kpm, 1.0)
    assert bool((o[L:] == 0).all()) and bool(torch.isfinite(o).all()) and float(o[:L].abs().min()) > 0
    p = R.softmax_masked(q, k, B, L, L, True, None)
    assert float((p.sum(-1) - 1).abs().max()) < 1e-14 and float(p[:, :, 0, 1:].abs().max()) == 0.0


def test_dropout_hash_restatement():
    """The pair convention (one hash for elements 2k, 2k + 1; low field = even element), the threshold p * 65536 + 0.5 and the rate."""
    idx = np.arange(1 << 20)
    for p in (0.1, 0.3, 0.5):
        m = R.drop_mult(7, 3, p, idx)
        assert set(np.unique(m)) == {0.0, float(np.float32(1) / (np.float32(1) - np.float32(p)))}
        assert abs((m == 0).mean() - p) < 4 * np.sqrt(p * (1 - p) / idx.size) + 1.0 / 65536
    # by hand for one pair: seed 7, site 3, elements 10 and 11 share the hash of pair 5
    M = 0xFFFFFFFF
    key = ((7 * 0x9E3779B1) & M) ^ ((3 * 0x85EBCA77 + 0x165667B1) & M)
    x = ((5 * 0x9E3779B1) & M) ^ key
    x ^= x >> 16; x = (x * 0x85EBCA6B) & M; x ^= x >> 13; x = (x * 0xC2B2AE35) & M; x ^= x >> 16
    thresh = int(np.float32(0.5) * np.float32(65536) + np.float32(0.5))
    want = [0.0 if (x & 0xFFFF) < thresh else 2.0, 0.0 if (x >> 16) < thresh else 2.0]
    assert list(R.drop_mult(7, 3, 0.5, np.array([10, 11]))) == want
    assert not np.array_equal(R.drop_mult(7, 3, 0.5, idx[:4096]), R.drop_mult(7, 4, 0.5, idx[:4096]))      # the site enters the key
    assert not np.array_equal(R.drop_mult(7, 3, 0.5, idx[:4096]), R.drop_mult(8, 3, 0.5, idx[:4096]))      # and so does the seed
    assert np.array_equal(R.drop_mult(7, 3, 0.5, idx[:64] + (1 << 32)), R.drop_mult(7, 3, 0.5, idx[:64]))  # counters are 32 bits wide
    assert bool((R.drop_mult(None, 3, 0.5, idx[:64]) == 1).all()) and bool((R.drop_mult(7, 3, 0.0, idx[:64]) == 1).all())


def test_prologues_equal_the_oracle():
    B, T, S, V = 3, 5, 6, 40
    rng = np.random.default_rng(5)
    p = {O.ENC + "unify.0.weight": rng.standard_normal((D, D)) * 0.05, O.ENC + "unify.0.bias": rng.standard_normal(D) * 0.1,
         O.ENC + "temp_emb.pe": O.encoder_pos_table(32, D).astype(np.float64),
         O.DEC + "tgt_to_emb.weight": rng.standard_normal((V, D)), O.DEC + "positional_encoding.pos_embedding": O.decoder_pos_table(32, D).astype(np.float64)}
    feats = rng.standard_normal((B, T, D))
    z, _ = O.encoder_frontend(p, feats, dt=np.float64)
    pe_rows = O.temporal_encoding_rows(p[O.ENC + "temp_emb.pe"], T)
    x, x_in = R.frontend(torch.from_numpy(feats).reshape(B * T, D), torch.from_numpy(p[O.ENC + "unify.0.weight"]),
                         torch.from_numpy(p[O.ENC + "unify.0.bias"]), torch.from_numpy(pe_rows), B, T)
    close("front end", x, torch.from_numpy(z).reshape(B * (T + 1), D), 1e-13)
    assert torch.equal(x_in, torch.from_numpy(feats).reshape(B * T, D))
    ids = rng.integers(0, V, (B, S + 2))
    e = O.embed_tokens(p, ids[:, :S], dt=np.float64)
    mine = R.embed(torch.from_numpy(ids), torch.from_numpy(p[O.DEC + "tgt_to_emb.weight"]),
                   torch.from_numpy(p[O.DEC + "positional_encoding.pos_embedding"]), B, S)
    close("embedding", mine, torch.from_numpy(e).reshape(B * S, D), 1e-13)


# ---- the stream order the GPU tests lay weights out in == the block lists the engine packs ----------------------------------------------
_NAMES = {"self_attn.in_proj_weight": "w_in", "self_attn.out_proj.weight": "w_o", "multihead_attn.in_proj_weight": "c_in",
          "multihead_attn.out_proj.weight": "c_o", "linear1.weight": "w1", "linear2.weight": "w2"}


class _FakeParams:
    def __init__(self, ff, lps):
        shapes = {"self_attn.in_proj_weight": (3 * D, D), "self_attn.out_proj.weight": (D, D), "multihead_attn.in_proj_weight": (3 * D, D),
                  "multihead_attn.out_proj.weight": (D, D), "linear1.weight": (ff, D), "linear2.weight": (D, ff)}
        self.c = {"S." + lp + n: torch.zeros(s, dtype=torch.bfloat16) for lp in lps for n, s in shapes.items()}
        self.c["S.unify.0.weight"] = torch.zeros(D, D, dtype=torch.bfloat16)

    def want_packed(self, key, parts):
        return parts

    def locate(self, view):
        """(name, row0, col0) of a view of one of the matrices."""
        for n, m in self.c.items():
            if view.untyped_storage().data_ptr() == m.untyped_storage().data_ptr():
                assert view.stride(0) == m.shape[1] and view.stride(1) == 1, n
                off = view.storage_offset() - m.storage_offset()
                return n, off // m.shape[1], off % m.shape[1]
        raise AssertionError("a block that is no view of a weight")


class _FakeStack:
    pre = "S."

    def __init__(self, ff, lps):
        self.cfg, self.ps = {"ff": ff}, _FakeParams(ff, lps)


def _engine_table(fake, part, lp):
    out = []
    for blk in part[1]():
        name, r0, c0 = fake.ps.locate(blk[0])
        assert name.startswith("S." + lp), (name, lp)
        out.append((_NAMES[name[len("S." + lp):]], r0, c0, blk[1], blk[2], bool(blk[3]) if len(blk) > 3 else False))
    return out


@pytest.mark.parametrize("ff", [512, 2048])
@pytest.mark.parametrize("cross", [False, True])
def test_stream_tables_equal_the_engines_block_lists(ff, cross):
    from vct_amd.engine.stack import _StackBase
    lps = ["layers.0.", "layers.1."]
    fake = _FakeStack(ff, lps)
    parts = _StackBase._ss_stream(fake, lps, cross, lead=None if cross else "unify.0.weight")
    if not cross:
        lead = parts.pop(0)
        (v, nch, at), = lead[1]()
        assert fake.ps.locate(v) == ("S.unify.0.weight", 0, 0) and (nch, at) == (8, 0)
    assert len(parts) == 2
    per = 8 * (4 + (4 if cross else 0) + 2 * (ff // 512))
    for part, lp in zip(parts, lps):
        table = R.fwd_stream_table(ff, cross)
        assert _engine_table(fake, part, lp) == table
        assert max(t[4] + t[3] for t in table) == per and sorted(t[4] for t in table) == list(range(0, per, 8))
    if not cross:
        parts = _StackBase._ss_stream_bwd(fake, lps)
        per = 8 * (2 * (ff // 512) + 4)
        for part, lp in zip(parts, lps):
            table = R.bwd_stream_table(ff)
            assert _engine_table(fake, part, lp) == table
            assert max(t[4] + t[3] for t in table) == per and all(t[5] for t in table)


def test_stream_tables_follow_the_header_text():
    """include/vct_hip.h by hand for ff = 1024: in_proj rows [0,512) [512,1024) [1024,1536) | out_proj | cross in_proj x3 | cross out_proj |
    linear1 rows [0,512) | linear1 rows [512,1024) , linear2 columns [0,512) | linear2 columns [512,1024)."""
    t = [(n, r, c, a) for n, r, c, _, a, _ in R.fwd_stream_table(1024, True)]
    assert t == [("w_in", 0, 0, 0), ("w_in", 512, 0, 8), ("w_in", 1024, 0, 16), ("w_o", 0, 0, 24), ("c_in", 0, 0, 32), ("c_in", 512, 0, 40),
                 ("c_in", 1024, 0, 48), ("c_o", 0, 0, 56), ("w1", 0, 0, 64), ("w1", 512, 0, 72), ("w2", 0, 0, 80), ("w2", 0, 512, 88)]
    b = [(n, r, c, k, a) for n, r, c, k, a, _ in R.bwd_stream_table(1024)]
    assert b == [("w2", 0, 0, 8, 0), ("w1", 0, 0, 8, 8), ("w2", 0, 512, 8, 16), ("w1", 512, 0, 8, 24), ("w_o", 0, 0, 8, 32), ("w_in", 0, 0, 24, 40)]


def test_packed_block_restatement():
    """Lane l of fragment (wave, tile, k-step) of chunk c <- A[64 wave + 16 tile + (l & 15)][64 c + 32 k-step + 8 (l >> 4) ..]; transposed: A = src^T."""
    src = np.arange(512 * 128, dtype=np.int16).reshape(512, 128)
    pk = R.packed_block(src, 2, False)
    assert pk[1, 3, 2, 1, 37, 5] == src[3 * 64 + 2 * 16 + 5, 64 + 32 + 2 * 8 + 5]
    srct = np.arange(128 * 512, dtype=np.int16).reshape(128, 512)
    pk = R.packed_block(srct, 2, True)
    assert pk[1, 3, 2, 1, 37, 5] == srct[64 + 32 + 2 * 8 + 5, 3 * 64 + 2 * 16 + 5]
