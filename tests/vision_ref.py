"""Restatement of CLIP's image path, the definition of vct_amd.vision.ClipVisionTower.  numpy / plain torch in float64; nothing here
reads the library or vct_amd.  tests/test_vision_tower_cpu.py checks THIS file against PIL and transformers.CLIPVisionModelWithProjection;
tests/test_vision_tower_gpu.py checks the kernels against it.

    image = Normalize(ToTensor(CenterCrop(R)(Resize(R, BICUBIC)(frame))))           (clip/clip.py, _transform)
    e = patches(image) @ conv1.weight.view(W, 3 P P)^T;  s = [class_embedding; e] + positional_embedding;  x = ln_pre(s)
    per layer:  x = x + out_proj(MHA(ln_1(x)));  x = x + c_proj(QuickGELU(c_fc(ln_2(x))))     (no mask, scores / sqrt(hd))
    y = ln_post(x[:, 0]) @ proj                                                     LayerNorm eps 1e-5

The resize is PIL's (src/libImaging/Resample.c, 8 bits per channel): per output index a window and fp64 weights of the a = -0.5 cubic
over a support of 2 max(scale, 1), normalised, rounded half away from zero to 22-bit fixed point; an accumulator that starts at 2^21,
is shifted right by 22 and clamped to 0 .. 255; the horizontal pass first, the vertical pass on its uint8 result; a pass whose size
does not change is skipped.

emulate=True rounds where the kernels round (tests/text_tower_ref.py's convention): the patch matrix, the GEMM weights, every LayerNorm
output but ln_pre's (which IS the fp32 stream), q / k / v, the probabilities, the attention output, the activation output and the
pooled row to bf16; the patch GEMM's output and the stream to fp32.

The check_* functions are what the GPU file asserts with; the CPU file feeds them seeded faults."""
import math

import numpy as np
import torch

import text_tower_ref as T

F64 = torch.float64
PB = 22
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
# the seven sizes on which the integer resize was compared with PIL byte by byte: (H, W, R)
SIZES = [(360, 640, 224), (240, 320, 224), (480, 270, 224), (100, 37, 32), (32, 32, 32), (50, 200, 32), (20, 31, 32)]


# ---- PIL's resize ---------------------------------------------------------------------------------------------------------------------
def bicubic(x, a=-0.5):
    x = abs(x)
    if x < 1:
        return ((a + 2) * x - (a + 3)) * x * x + 1
    if x < 2:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def coeffs(in_size, out_size):
    """-> [(xmin, int64 weights)] for every output index of one pass."""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support, ss = 2.0 * fs, 1.0 / fs
    out = []
    for xx in range(out_size):
        c = (xx + 0.5) * scale
        xmin = max(int(c - support + 0.5), 0)
        xmax = min(int(c + support + 0.5), in_size)
        w = [bicubic((x + xmin - c + 0.5) * ss) for x in range(xmax - xmin)]
        ww = sum(w)
        w = [v / ww for v in w]
        k = [int(-0.5 + v * (1 << PB)) if v < 0 else int(0.5 + v * (1 << PB)) for v in w]
        out.append((xmin, np.array(k, dtype=np.int64)))
    return out


def pass1d(img, out_size, cs=None):
    """One pass along axis 1 of a uint8 [H, W, C] image."""
    H, W, C = img.shape
    cs = coeffs(W, out_size) if cs is None else cs
    o = np.empty((H, out_size, C), np.uint8)
    for xx, (x0, k) in enumerate(cs):
        acc = (img[:, x0:x0 + len(k), :].astype(np.int64) * k[None, :, None]).sum(1) + (1 << (PB - 1))
        o[:, xx, :] = np.clip(acc >> PB, 0, 255)
    return o


def resize(img, oh, ow):
    """PIL.Image.resize((ow, oh), BICUBIC) of a uint8 [H, W, C] image."""
    t = pass1d(img, ow) if ow != img.shape[1] else img
    if oh != img.shape[0]:
        t = pass1d(t.transpose(1, 0, 2), oh).transpose(1, 0, 2)
    return t


def resized_size(H, W, R):
    return (R, int(R * W / H)) if H <= W else (int(R * H / W), R)


def crop_offsets(oh, ow, R):
    return int(round((oh - R) / 2.0)), int(round((ow - R) / 2.0))


def preprocess_u8(img, R):
    """Resize(R, BICUBIC) + CenterCrop(R) of a uint8 [H, W, 3] frame -> uint8 [R, R, 3]."""
    oh, ow = resized_size(img.shape[0], img.shape[1], R)
    top, left = crop_offsets(oh, ow, R)
    return np.ascontiguousarray(resize(img, oh, ow)[top:top + R, left:left + R])


def pil_preprocess_u8(img, R):
    """The same through PIL itself (the arbiter)."""
    from PIL import Image
    oh, ow = resized_size(img.shape[0], img.shape[1], R)
    top, left = crop_offsets(oh, ow, R)
    im = Image.fromarray(img).resize((ow, oh), Image.BICUBIC).crop((left, top, left + R, top + R))
    return np.ascontiguousarray(np.asarray(im))


def tables(H, W, R):
    """The form the kernel takes: windows and padded weights of the R cropped columns / rows only; a skipped pass is the one-tap
    table of weight 2^22.  -> dict(hx_min, hx_len, hx_w, vy_min, vy_len, vy_w), int32."""
    oh, ow = resized_size(H, W, R)
    top, left = crop_offsets(oh, ow, R)
    out = {}
    for name, n_in, n_out, first in (("hx", W, ow, left), ("vy", H, oh, top)):
        if n_in == n_out:
            cs = [(i, np.array([1 << PB], np.int64)) for i in range(first, first + R)]
        else:
            cs = coeffs(n_in, n_out)[first:first + R]
        k = max(len(c[1]) for c in cs)
        w = np.zeros((R, k), np.int32)
        for i, c in enumerate(cs):
            w[i, :len(c[1])] = c[1]
        out[name + "_min"], out[name + "_len"], out[name + "_w"] = (np.array([c[0] for c in cs], np.int32),
                                                                    np.array([len(c[1]) for c in cs], np.int32), w)
    return out


def value_table(mean=CLIP_MEAN, std=CLIP_STD, dtype=torch.float32):
    """ToTensor + Normalize of every byte as torchvision computes them: uint8 -> fp32, `.div(255)`, `.sub_(mean).div_(std)` with fp32
    mean / std [3, 1, 1] -- here on a [3, 256, 1] "image" whose rows are the bytes.  -> [3, 256]."""
    img = torch.arange(256, dtype=torch.uint8).view(1, 256, 1).expand(3, 256, 1)
    t = img.to(torch.float32).div(255)
    m = torch.as_tensor(mean, dtype=torch.float32).view(-1, 1, 1)
    s = torch.as_tensor(std, dtype=torch.float32).view(-1, 1, 1)
    return t.clone().sub_(m).div_(s).view(3, 256).to(dtype)


def patch_matrix(crop, lut, P):
    """crop uint8 [N, R, R, 3] (numpy or torch), lut [3, 256] -> [N * G * G, 3 P P] in lut's dtype: row (n, gy, gx), column
    (c, py, px) -- conv1.weight.view(W, 3 P P)'s layout."""
    crop = torch.as_tensor(crop).to(lut.device)
    N, R = crop.shape[0], crop.shape[1]
    G = R // P
    img = torch.stack([lut[c][crop[..., c].long()] for c in range(3)], 1)                 # [N, 3, R, R]
    return img.view(N, 3, G, P, G, P).permute(0, 2, 4, 1, 3, 5).reshape(N * G * G, 3 * P * P).contiguous()


# ---- the tower ------------------------------------------------------------------------------------------------------------------------
def _d(t):
    return torch.as_tensor(t).detach().to("cpu").to(F64)


def weights(sd, prefix=""):
    """-> dict(conv [W, 3 P P], patch, cls, pos, lnpre_g, lnpre_b, layers=[...], lnpost_g, lnpost_b, proj [W, P_out]) in fp64, from
    either key convention."""
    if prefix:
        sd = {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}
    if "visual.conv1.weight" in sd:
        layers, l = [], 0
        while f"visual.transformer.resblocks.{l}.ln_1.weight" in sd:
            q = f"visual.transformer.resblocks.{l}."
            layers.append(dict(ln1_g=_d(sd[q + "ln_1.weight"]), ln1_b=_d(sd[q + "ln_1.bias"]),
                               w_qkv=_d(sd[q + "attn.in_proj_weight"]), b_qkv=_d(sd[q + "attn.in_proj_bias"]),
                               w_o=_d(sd[q + "attn.out_proj.weight"]), b_o=_d(sd[q + "attn.out_proj.bias"]),
                               ln2_g=_d(sd[q + "ln_2.weight"]), ln2_b=_d(sd[q + "ln_2.bias"]),
                               w_fc=_d(sd[q + "mlp.c_fc.weight"]), b_fc=_d(sd[q + "mlp.c_fc.bias"]),
                               w_proj=_d(sd[q + "mlp.c_proj.weight"]), b_proj=_d(sd[q + "mlp.c_proj.bias"])))
            l += 1
        conv = _d(sd["visual.conv1.weight"])
        return dict(conv=conv.reshape(conv.shape[0], -1), patch=conv.shape[2], cls=_d(sd["visual.class_embedding"]),
                    pos=_d(sd["visual.positional_embedding"]), lnpre_g=_d(sd["visual.ln_pre.weight"]), lnpre_b=_d(sd["visual.ln_pre.bias"]),
                    layers=layers, lnpost_g=_d(sd["visual.ln_post.weight"]), lnpost_b=_d(sd["visual.ln_post.bias"]), proj=_d(sd["visual.proj"]))
    p = "vision_model."
    layers, l = [], 0
    while p + f"encoder.layers.{l}.layer_norm1.weight" in sd:
        q = p + f"encoder.layers.{l}."
        layers.append(dict(ln1_g=_d(sd[q + "layer_norm1.weight"]), ln1_b=_d(sd[q + "layer_norm1.bias"]),
                           w_qkv=torch.cat([_d(sd[q + f"self_attn.{x}_proj.weight"]) for x in "qkv"], 0),
                           b_qkv=torch.cat([_d(sd[q + f"self_attn.{x}_proj.bias"]) for x in "qkv"], 0),
                           w_o=_d(sd[q + "self_attn.out_proj.weight"]), b_o=_d(sd[q + "self_attn.out_proj.bias"]),
                           ln2_g=_d(sd[q + "layer_norm2.weight"]), ln2_b=_d(sd[q + "layer_norm2.bias"]),
                           w_fc=_d(sd[q + "mlp.fc1.weight"]), b_fc=_d(sd[q + "mlp.fc1.bias"]),
                           w_proj=_d(sd[q + "mlp.fc2.weight"]), b_proj=_d(sd[q + "mlp.fc2.bias"])))
        l += 1
    conv = _d(sd[p + "embeddings.patch_embedding.weight"])
    return dict(conv=conv.reshape(conv.shape[0], -1), patch=conv.shape[2], cls=_d(sd[p + "embeddings.class_embedding"]),
                pos=_d(sd[p + "embeddings.position_embedding.weight"]), lnpre_g=_d(sd[p + "pre_layrnorm.weight"]),
                lnpre_b=_d(sd[p + "pre_layrnorm.bias"]), layers=layers, lnpost_g=_d(sd[p + "post_layernorm.weight"]),
                lnpost_b=_d(sd[p + "post_layernorm.bias"]), proj=_d(sd["visual_projection.weight"]).t())


def attention(qkv, B, L, H, r=T.ident):
    """qkv [B * L, 3 W] (as stored) -> [B * L, W]: softmax(q k^T / sqrt(hd)) v per head, no mask; r rounds the probabilities."""
    W = qkv.shape[1] // 3
    hd = W // H
    sp = lambda t: t.reshape(B, L, H, hd).transpose(1, 2)      # noqa: E731
    q, k, v = (sp(qkv[:, i * W:(i + 1) * W]) for i in range(3))
    s = q @ k.transpose(-1, -2) / math.sqrt(hd)
    return (r(torch.softmax(s, -1)) @ v).transpose(1, 2).reshape(B * L, W)


def embed(e, cls, pos, g, b):
    """e [N * (L - 1), W] -> ln_pre([cls; e_n] + pos) as [N * L, W]."""
    L = pos.shape[0]
    N = e.shape[0] // (L - 1)
    s = torch.cat([cls.expand(N, 1, -1), e.reshape(N, L - 1, -1)], 1) + pos
    return T.layer_norm(s, g, b).reshape(N * L, -1)


def pool(x, L, g, b):
    return T.layer_norm(x.reshape(-1, L, x.shape[1])[:, 0], g, b)


def tower(sd, frames, heads, mean=CLIP_MEAN, std=CLIP_STD, emulate=False, keep=False, prefix=""):
    """frames: uint8 [N, H, W, 3] (numpy or torch) -> fp64 [N, P_out].  keep: also every intermediate, named as
    ClipVisionTower.encode_frames(keep=True) names them."""
    w = weights(sd, prefix)
    frames = np.asarray(torch.as_tensor(frames).cpu())
    P, L = w["patch"], w["pos"].shape[0]
    R = math.isqrt(L - 1) * P
    crop = np.stack([preprocess_u8(f, R) for f in frames])
    r, s32 = (T.bf, T.f32) if emulate else (T.ident, T.ident)
    a = r(patch_matrix(crop, value_table(mean, std), P).to(F64))
    e = s32(a @ r(w["conv"]).t())
    x = s32(embed(e, w["cls"], w["pos"], w["lnpre_g"], w["lnpre_b"]))
    N = frames.shape[0]
    kept = dict(crop=torch.from_numpy(crop), a=a, e=e, x0=x, layers=[])
    for lw in w["layers"]:
        h1 = r(T.layer_norm(x, lw["ln1_g"], lw["ln1_b"]))
        qkv = r(h1 @ r(lw["w_qkv"]).t() + lw["b_qkv"])
        o = r(attention(qkv, N, L, heads, r))
        x1 = s32(x + o @ r(lw["w_o"]).t() + lw["b_o"])
        h2 = r(T.layer_norm(x1, lw["ln2_g"], lw["ln2_b"]))
        f = r(T.quick_gelu(h2 @ r(lw["w_fc"]).t() + lw["b_fc"]))
        x = s32(x1 + f @ r(lw["w_proj"]).t() + lw["b_proj"])
        kept["layers"].append(dict(h1=h1, qkv=qkv, o=o, x1=x1, h2=h2, f=f, x2=x))
    pooled = r(pool(x, L, w["lnpost_g"], w["lnpost_b"]))
    out = pooled @ r(w["proj"])
    kept.update(pooled=pooled, out=out)
    return (out, kept) if keep else out


# ---- test models ----------------------------------------------------------------------------------------------------------------------
def random_state_dict(W, ff, layers, P_out, patch, R, seed, std=0.08, convention="openai", prefix=""):
    """A random tower in OpenAI's key convention (fp32 values; LayerNorm gains around 1) or, with convention="transformers", the same
    weights under transformers' keys; `prefix` goes in front of every key."""
    g = torch.Generator().manual_seed(seed)
    n = lambda *s, sc=std: (torch.randn(*s, generator=g) * sc).to(torch.float32)      # noqa: E731
    L = (R // patch) ** 2 + 1
    v = "visual."
    sd = {v + "conv1.weight": n(W, 3, patch, patch, sc=(3 * patch * patch) ** -0.5), v + "class_embedding": n(W, sc=0.5),
          v + "positional_embedding": n(L, W, sc=0.3), v + "ln_pre.weight": 1 + n(W, sc=0.1), v + "ln_pre.bias": n(W, sc=0.1),
          v + "ln_post.weight": 1 + n(W, sc=0.1), v + "ln_post.bias": n(W, sc=0.1), v + "proj": n(W, P_out, sc=W ** -0.5),
          "logit_scale": torch.tensor(4.6), "token_embedding.weight": n(4, 4)}          # the last two must be ignored by a loader
    for l in range(layers):
        q = v + f"transformer.resblocks.{l}."
        sd.update({q + "ln_1.weight": 1 + n(W, sc=0.1), q + "ln_1.bias": n(W, sc=0.1), q + "ln_2.weight": 1 + n(W, sc=0.1),
                   q + "ln_2.bias": n(W, sc=0.1), q + "attn.in_proj_weight": n(3 * W, W), q + "attn.in_proj_bias": n(3 * W, sc=0.1),
                   q + "attn.out_proj.weight": n(W, W), q + "attn.out_proj.bias": n(W, sc=0.1),
                   q + "mlp.c_fc.weight": n(ff, W), q + "mlp.c_fc.bias": n(ff, sc=0.1),
                   q + "mlp.c_proj.weight": n(W, ff), q + "mlp.c_proj.bias": n(W, sc=0.1)})
    if convention != "openai":
        sd = openai_to_transformers(sd)
    return {prefix + k: t for k, t in sd.items()}


def openai_to_transformers(sd):
    p, v = "vision_model.", "visual."
    out = {p + "embeddings.patch_embedding.weight": sd[v + "conv1.weight"], p + "embeddings.class_embedding": sd[v + "class_embedding"],
           p + "embeddings.position_embedding.weight": sd[v + "positional_embedding"],
           p + "pre_layrnorm.weight": sd[v + "ln_pre.weight"], p + "pre_layrnorm.bias": sd[v + "ln_pre.bias"],
           p + "post_layernorm.weight": sd[v + "ln_post.weight"], p + "post_layernorm.bias": sd[v + "ln_post.bias"],
           "visual_projection.weight": sd[v + "proj"].t().contiguous()}
    W = sd[v + "conv1.weight"].shape[0]
    l = 0
    while v + f"transformer.resblocks.{l}.ln_1.weight" in sd:
        a, b = v + f"transformer.resblocks.{l}.", p + f"encoder.layers.{l}."
        for i, x in enumerate("qkv"):
            out[b + f"self_attn.{x}_proj.weight"] = sd[a + "attn.in_proj_weight"][i * W:(i + 1) * W].clone()
            out[b + f"self_attn.{x}_proj.bias"] = sd[a + "attn.in_proj_bias"][i * W:(i + 1) * W].clone()
        for src, dst in (("attn.out_proj", "self_attn.out_proj"), ("ln_1", "layer_norm1"), ("ln_2", "layer_norm2"),
                         ("mlp.c_fc", "mlp.fc1"), ("mlp.c_proj", "mlp.fc2")):
            out[b + dst + ".weight"], out[b + dst + ".bias"] = sd[a + src + ".weight"], sd[a + src + ".bias"]
        l += 1
    return out


def random_frames(N, H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (N, H, W, 3), dtype=np.uint8)


# ---- the checkers of the GPU file ------------------------------------------------------------------------------------------------------
U = {torch.bfloat16: 2.0 ** -8, torch.float32: 2.0 ** -24}


def ln_bound(ref, dtype):
    """tests/test_text_tower_gpu.py's LayerNorm bound: fp32 arithmetic on a given row, u |ref| + 2e-5 max |ref| per element."""
    return U[dtype] * ref.abs() + 2e-5 * ref.abs().max()


def check_crop(got, frames, R, arbiter=pil_preprocess_u8):
    """got uint8 [N, R, R, 3] equals the arbiter's resize + crop of every frame in every byte."""
    got = np.asarray(torch.as_tensor(got).cpu())
    frames = np.asarray(torch.as_tensor(frames).cpu())
    assert got.shape == (frames.shape[0], R, R, 3) and got.dtype == np.uint8, (got.shape, got.dtype)
    for n, f in enumerate(frames):
        ref = arbiter(f, R)
        bad = int((ref != got[n]).sum())
        assert bad == 0, f"frame {n}: {bad} of {ref.size} bytes of the cropped image differ from PIL's"


def check_patches(got, crop, lut, P):
    """got [N G G, 3 P P] equals lut[crop] rearranged in every bit."""
    ref = patch_matrix(crop, lut.to(got.device), P)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (got.shape, got.dtype)
    same = got.contiguous().view(torch.uint8) == ref.view(torch.uint8)
    assert bool(same.all()), f"{int((~same).sum())} bytes of the patch matrix differ from lut[crop]"


def check_elem(what, got, ref, bnd):
    excess = torch.nan_to_num(((got.detach().to(F64) - ref).abs() - bnd), nan=float("inf"))
    worst = float(excess.max())
    print(f"[vision-tower] {what}: worst |got - ref| - bound = {worst:.3e}; max |got - ref| = {float((got.detach().to(F64) - ref).abs().max()):.3e}")
    assert worst <= 0.0, (what, worst)


def check_embed(what, got, e, cls, pos, g, b):
    """got fp32 [N L, W] against ln_pre([cls; e] + pos) in fp64 of the operands as stored, to the LayerNorm bound (the sum's own fp32
    rounding, u |s|, passes through the norm with a gain of at most |gamma| rstd and is inside the 2e-5 term for O(1) rows)."""
    d = lambda t: t.detach().to(F64)      # noqa: E731
    ref = embed(d(e), d(cls), d(pos), d(g), d(b))
    assert tuple(got.shape) == tuple(ref.shape), (got.shape, ref.shape)
    check_elem(what, got, ref.to(got.device), ln_bound(ref, torch.float32).to(got.device))


def check_pool(what, got, x, L, g, b):
    """got [N, W] against ln_post of the class rows x[n L] in fp64, to the LayerNorm bound of got's dtype."""
    d = lambda t: t.detach().to(F64)      # noqa: E731
    rows = d(x).reshape(-1, L, x.shape[1])[:, 0]
    ref = T.layer_norm(rows, d(g), d(b))
    assert tuple(got.shape) == tuple(ref.shape), (got.shape, ref.shape)
    check_elem(what, got, ref, ln_bound(ref, got.dtype))
