"""fp64 restatement of OpenAI CLIP's `encode_text` (clip/model.py), the definition of vct_amd.text.ClipTextTower.  Plain torch
in float64; nothing here reads the library or vct_amd.  tests/test_text_tower_cpu.py checks THIS file against
transformers.CLIPTextModelWithProjection; tests/test_text_tower_gpu.py checks the kernels against it.

    x = token_embedding[ids] + positional_embedding[:L]
    per layer:  x = x + out_proj(MHA(ln_1(x), causal, scores / sqrt(hd)));  x = x + c_proj(QuickGELU(c_fc(ln_2(x))))
    y = ln_final(x)[b, e_b] @ text_projection,      e_b = FIRST index of the maximum of ids[b],  LayerNorm eps 1e-5

Both key conventions are read (weights(): OpenAI's `clip.load(...).state_dict()` and transformers'), by a mapping written here and not
shared with the package.

emulate=True rounds to bf16 where the kernels do: the GEMM weights, both LayerNorm outputs, q / k / v, the probabilities, the attention
output, the activation output and the pooled row; the stream (embedding sum and both residual sums) is rounded to fp32.  It states
WHERE roundings happen, it is not a bit-exact model of the kernels (accumulation order, exp and rcp differ)."""
import math

import torch

F64 = torch.float64


def _d(t):
    return torch.as_tensor(t).detach().to("cpu").to(F64)


def weights(sd):
    """-> dict(tok, pos, layers=[dict(ln1_g, ln1_b, w_qkv, b_qkv, w_o, b_o, ln2_g, ln2_b, w_fc, b_fc, w_proj, b_proj)], lnf_g, lnf_b,
    proj [W, P]) in fp64, from either key convention."""
    if "token_embedding.weight" in sd:
        n = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("transformer.resblocks."))
        layers = []
        for l in range(n):
            q = f"transformer.resblocks.{l}."
            layers.append(dict(ln1_g=_d(sd[q + "ln_1.weight"]), ln1_b=_d(sd[q + "ln_1.bias"]),
                               w_qkv=_d(sd[q + "attn.in_proj_weight"]), b_qkv=_d(sd[q + "attn.in_proj_bias"]),
                               w_o=_d(sd[q + "attn.out_proj.weight"]), b_o=_d(sd[q + "attn.out_proj.bias"]),
                               ln2_g=_d(sd[q + "ln_2.weight"]), ln2_b=_d(sd[q + "ln_2.bias"]),
                               w_fc=_d(sd[q + "mlp.c_fc.weight"]), b_fc=_d(sd[q + "mlp.c_fc.bias"]),
                               w_proj=_d(sd[q + "mlp.c_proj.weight"]), b_proj=_d(sd[q + "mlp.c_proj.bias"])))
        return dict(tok=_d(sd["token_embedding.weight"]), pos=_d(sd["positional_embedding"]), layers=layers,
                    lnf_g=_d(sd["ln_final.weight"]), lnf_b=_d(sd["ln_final.bias"]), proj=_d(sd["text_projection"]))
    p = "text_model."
    n = 1 + max(int(k.split(".")[3]) for k in sd if k.startswith(p + "encoder.layers."))
    layers = []
    for l in range(n):
        q = p + f"encoder.layers.{l}."
        layers.append(dict(ln1_g=_d(sd[q + "layer_norm1.weight"]), ln1_b=_d(sd[q + "layer_norm1.bias"]),
                           w_qkv=torch.cat([_d(sd[q + f"self_attn.{x}_proj.weight"]) for x in "qkv"], 0),
                           b_qkv=torch.cat([_d(sd[q + f"self_attn.{x}_proj.bias"]) for x in "qkv"], 0),
                           w_o=_d(sd[q + "self_attn.out_proj.weight"]), b_o=_d(sd[q + "self_attn.out_proj.bias"]),
                           ln2_g=_d(sd[q + "layer_norm2.weight"]), ln2_b=_d(sd[q + "layer_norm2.bias"]),
                           w_fc=_d(sd[q + "mlp.fc1.weight"]), b_fc=_d(sd[q + "mlp.fc1.bias"]),
                           w_proj=_d(sd[q + "mlp.fc2.weight"]), b_proj=_d(sd[q + "mlp.fc2.bias"])))
    return dict(tok=_d(sd[p + "embeddings.token_embedding.weight"]), pos=_d(sd[p + "embeddings.position_embedding.weight"]),
                layers=layers, lnf_g=_d(sd[p + "final_layer_norm.weight"]), lnf_b=_d(sd[p + "final_layer_norm.bias"]),
                proj=_d(sd["text_projection.weight"]).t())


# ---- the stages, each usable on its own (the GPU file recomputes every stored intermediate from the one stored before it) -------------
def bf(t):
    return t.to(torch.float32).to(torch.bfloat16).to(F64)


def f32(t):
    return t.to(torch.float32).to(F64)


def ident(t):
    return t


def layer_norm(x, g, b):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + 1e-5) * g + b


def quick_gelu(v):
    return v * torch.sigmoid(1.702 * v)


def first_argmax(ids):
    """First index of each row's maximum, by an explicit scan (torch.argmax documents no tie rule)."""
    out = []
    for row in torch.as_tensor(ids).tolist():
        best, at = row[0], 0
        for i, v in enumerate(row):
            if v > best:
                best, at = v, i
        out.append(at)
    return torch.tensor(out, dtype=torch.int64)


def attention(qkv, B, L, H, r=ident):
    """qkv [B * L, 3 W] (as stored) -> [B * L, W]: causal softmax(q k^T / sqrt(hd)) v per head; r rounds the probabilities."""
    W = qkv.shape[1] // 3
    hd = W // H
    sp = lambda t: t.reshape(B, L, H, hd).transpose(1, 2)      # noqa: E731
    q, k, v = (sp(qkv[:, i * W:(i + 1) * W]) for i in range(3))
    s = q @ k.transpose(-1, -2) / math.sqrt(hd)
    s = s + torch.triu(torch.full((L, L), float("-inf"), dtype=F64, device=qkv.device), 1)
    return (r(torch.softmax(s, -1)) @ v).transpose(1, 2).reshape(B * L, W)


def tower(sd, ids, heads, L=None, emulate=False, keep=False):
    """ids int [B, n] -> fp64 [B, P].  L: run only the first L positions (None: all n; the maximum must lie inside).  keep: also
    return every intermediate, named as ClipTextTower.encode_ids(keep=True) names them."""
    w = weights(sd)
    ids = torch.as_tensor(ids).to(torch.int64)
    e = first_argmax(ids)
    B = ids.shape[0]
    L = ids.shape[1] if L is None else L
    assert int(e.max()) < L, "the trim cut an end-of-text token off"
    r, s32 = (bf, f32) if emulate else (ident, ident)
    x = s32(w["tok"][ids[:, :L]] + w["pos"][:L]).reshape(B * L, -1)
    kept = dict(x0=x, layers=[])
    for lw in w["layers"]:
        h1 = r(layer_norm(x, lw["ln1_g"], lw["ln1_b"]))
        qkv = r(h1 @ r(lw["w_qkv"]).t() + lw["b_qkv"])
        o = r(attention(qkv, B, L, heads, r))
        x1 = s32(x + o @ r(lw["w_o"]).t() + lw["b_o"])
        h2 = r(layer_norm(x1, lw["ln2_g"], lw["ln2_b"]))
        f = r(quick_gelu(h2 @ r(lw["w_fc"]).t() + lw["b_fc"]))
        x = s32(x1 + f @ r(lw["w_proj"]).t() + lw["b_proj"])
        kept["layers"].append(dict(h1=h1, qkv=qkv, o=o, x1=x1, h2=h2, f=f, x2=x))
    rows = x.reshape(B, L, -1)[torch.arange(B), e]
    pooled = r(layer_norm(rows, w["lnf_g"], w["lnf_b"]))
    out = pooled @ r(w["proj"])
    kept.update(pooled=pooled, eot=e, out=out)
    return (out, kept) if keep else out


# ---- test models -------------------------------------------------------------------------------------------------------------------------
def random_state_dict(W, H, ff, layers, P, vocab, seed, std=0.08, positions=77, convention="openai"):
    """A random tower in OpenAI's key convention (fp32 values; LayerNorm gains around 1, everything else N(0, std)) or, with
    convention="transformers", the same weights under transformers' keys."""
    g = torch.Generator().manual_seed(seed)
    n = lambda *s, sc=std: (torch.randn(*s, generator=g) * sc).to(torch.float32)      # noqa: E731
    sd = {"token_embedding.weight": n(vocab, W, sc=0.5), "positional_embedding": n(positions, W, sc=0.3),
          "ln_final.weight": 1 + n(W, sc=0.1), "ln_final.bias": n(W, sc=0.1), "text_projection": n(W, P, sc=W ** -0.5),
          "logit_scale": torch.tensor(4.6), "visual.proj": n(4, 4)}          # the last two must be ignored by a loader
    for l in range(layers):
        q = f"transformer.resblocks.{l}."
        sd.update({q + "ln_1.weight": 1 + n(W, sc=0.1), q + "ln_1.bias": n(W, sc=0.1), q + "ln_2.weight": 1 + n(W, sc=0.1),
                   q + "ln_2.bias": n(W, sc=0.1), q + "attn.in_proj_weight": n(3 * W, W), q + "attn.in_proj_bias": n(3 * W, sc=0.1),
                   q + "attn.out_proj.weight": n(W, W), q + "attn.out_proj.bias": n(W, sc=0.1),
                   q + "mlp.c_fc.weight": n(ff, W), q + "mlp.c_fc.bias": n(ff, sc=0.1),
                   q + "mlp.c_proj.weight": n(W, ff), q + "mlp.c_proj.bias": n(W, sc=0.1)})
    return sd if convention == "openai" else openai_to_transformers(sd)


def openai_to_transformers(sd):
    p = "text_model."
    out = {p + "embeddings.token_embedding.weight": sd["token_embedding.weight"],
           p + "embeddings.position_embedding.weight": sd["positional_embedding"],
           p + "final_layer_norm.weight": sd["ln_final.weight"], p + "final_layer_norm.bias": sd["ln_final.bias"],
           "text_projection.weight": sd["text_projection"].t().contiguous()}
    W = sd["token_embedding.weight"].shape[1]
    l = 0
    while f"transformer.resblocks.{l}.ln_1.weight" in sd:
        a, b = f"transformer.resblocks.{l}.", p + f"encoder.layers.{l}."
        for i, x in enumerate("qkv"):
            out[b + f"self_attn.{x}_proj.weight"] = sd[a + "attn.in_proj_weight"][i * W:(i + 1) * W].clone()
            out[b + f"self_attn.{x}_proj.bias"] = sd[a + "attn.in_proj_bias"][i * W:(i + 1) * W].clone()
        for src, dst in (("attn.out_proj", "self_attn.out_proj"), ("ln_1", "layer_norm1"), ("ln_2", "layer_norm2"),
                         ("mlp.c_fc", "mlp.fc1"), ("mlp.c_proj", "mlp.fc2")):
            out[b + dst + ".weight"], out[b + dst + ".bias"] = sd[a + src + ".weight"], sd[a + src + ".bias"]
        l += 1
    return out


def caption_ids(eots, vocab, seed, width=77):
    """int64 [B, width]: start token vocab - 2 at 0, random words, EOT (vocab - 1, the largest id) at index eots[b], zeros behind."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.zeros(len(eots), width, dtype=torch.int64)
    for b, e in enumerate(eots):
        ids[b, 0] = vocab - 2
        if e > 1:
            ids[b, 1:e] = torch.randint(1, vocab - 2, (e - 1,), generator=g)
        ids[b, e] = vocab - 1
    return ids
