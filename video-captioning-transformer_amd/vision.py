"""A frozen, forward-only CLIP vision tower on the library's kernels: uint8 frames -> fp32 [N, P_out] frame features.

The definition is OpenAI CLIP's `_transform` followed by `encode_image` (clip/clip.py, clip/model.py), which the reference reaches
from predict_video.py --video:

    image = Normalize(ToTensor(CenterCrop(R)(Resize(R, BICUBIC)(PIL image))))
    e = conv1(image) as a GEMM over P x P patches;   s = [class_embedding; e] + positional_embedding;   x = ln_pre(s)
    per layer:  x = x + out_proj(MHA(ln_1(x)));  x = x + c_proj(QuickGELU(c_fc(ln_2(x))))          (no mask)
    y = ln_post(x[:, 0]) @ proj

PIL's bicubic resize is integer arithmetic on 22-bit fixed-point weights, horizontal pass first and the vertical pass on its uint8
result.  The HOST builds the two coefficient tables in fp64 exactly as PIL does (resize_tables, cached per (H, W, R)) and the [3][256]
table of normalised values with torch's own fp32 ops (value_table); vct_frames_to_patches does integer taps and a lookup, so every
byte of the cropped image is PIL's and every element of the patch matrix is torch's.

Schedule: vct_frames_to_patches, vct_gemm (patch embedding, no bias, fp32 out), vct_vit_embed | the text tower's seven launches per
layer (text.run_layers, not causal) | vct_vit_pool, vct_gemm projection -> fp32: `7 layers + 5` launches.  The residual stream is fp32
in both modes; the GEMM operands are bf16 (rounded once, at load) or fp32 (parity mode).  Everything is enqueued on the current stream
through the runtime's launch wrapper; nothing synchronises.  L = (R / P)^2 + 1 rows per frame must fit the attention kernel's 64 keys:
ViT-B/32 at 224 px has 50; ViT-B/16 (197) and ViT-L/14 (257) are refused.  No video decoder, no frame-sampling policy and no weights
are shipped: the caller brings decoded uint8 frames and a CLIP (or CLIP4Clip, prefix="clip.") state dict."""
import functools
import math
import re
from typing import Dict, Optional

import numpy as np
import torch

from . import ops
from .text import _LAYER_KEYS, MAX_LEN, run_layers

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
PRECISION_BITS = 22      # PIL, 8-bit channels: 32 - 8 - 2


# ---- PIL's resize, restated for the host --------------------------------------------------------------------------------------------
def resized_size(H: int, W: int, R: int):
    """Resize(R): the shorter side becomes R, the longer int(R * long / short) -> (oh, ow)."""
    return (R, int(R * W / H)) if H <= W else (int(R * H / W), R)


def crop_offsets(oh: int, ow: int, R: int):
    """CenterCrop(R) of an oh x ow image -> (top, left); Python's round (half to even), as torchvision's."""
    return int(round((oh - R) / 2.0)), int(round((ow - R) / 2.0))


def _bicubic(x: float, a: float = -0.5) -> float:
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _pass_tables(in_size: int, out_size: int, first: int, count: int):
    """The windows and 22-bit weights of output indices first .. first + count of one resize pass in_size -> out_size, as PIL's
    precompute_coeffs / normalize_coeffs_8bpc compute them (fp64, the same operation order) -> (min [count], len [count], w [count, k])
    int32, w zero-padded to the widest window.  out_size == in_size: PIL skips the pass; the one-tap table of weight 2^22 says so."""
    if out_size == in_size:
        idx = np.arange(first, first + count, dtype=np.int32)
        return idx, np.ones(count, np.int32), np.full((count, 1), 1 << PRECISION_BITS, np.int32)
    scale = in_size / out_size
    fscale = max(scale, 1.0)
    support = 2.0 * fscale
    ss = 1.0 / fscale
    rows = []
    for xx in range(first, first + count):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [_bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        rows.append((xmin, [int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS)) for v in w]))
    k = max(len(r[1]) for r in rows)
    wts = np.zeros((count, k), np.int32)
    for i, (_m, r) in enumerate(rows):
        wts[i, :len(r)] = r
    return np.array([r[0] for r in rows], np.int32), np.array([len(r[1]) for r in rows], np.int32), wts


@functools.lru_cache(maxsize=64)
def resize_tables(H: int, W: int, R: int) -> dict:
    """Host tables of Resize(R, BICUBIC) + CenterCrop(R) for H x W frames: only the R cropped columns of the horizontal pass and the R
    cropped rows of the vertical one.  -> dict(R, oh, ow, top, left, hx_min, hx_len, hx_w [R, kx], vy_min, vy_len, vy_w [R, ky]),
    numpy int32; cached."""
    if H < 1 or W < 1 or R < 1:
        raise ValueError(f"CLIP vision tower: frames of {H} x {W} cannot be resized to {R}")
    oh, ow = resized_size(H, W, R)
    top, left = crop_offsets(oh, ow, R)
    hx = _pass_tables(W, ow, left, R)
    vy = _pass_tables(H, oh, top, R)
    return {"R": R, "oh": oh, "ow": ow, "top": top, "left": left, "hx_min": hx[0], "hx_len": hx[1], "hx_w": hx[2],
            "vy_min": vy[0], "vy_len": vy[1], "vy_w": vy[2]}


def stage_rows(tables: dict, P: int) -> int:
    """The largest number of input rows the P rows of one patch read: what vct_frames_to_patches stages in LDS."""
    lo, ln, R = tables["vy_min"], tables["vy_len"], tables["R"]
    return max(int(lo[g + P - 1] + ln[g + P - 1] - lo[g]) for g in range(0, R, P))


def value_table(mean, std, dtype=torch.float32) -> torch.Tensor:
    """[3, 256]: ToTensor + Normalize of every byte, per channel, with torch's own fp32 ops (`v / 255`, `- mean`, `/ std`), then torch's
    cast for bf16."""
    v = torch.arange(256, dtype=torch.float32).div(255)
    m, s = torch.tensor(mean, dtype=torch.float32), torch.tensor(std, dtype=torch.float32)
    return v[None, :].sub(m[:, None]).div(s[:, None]).to(dtype).contiguous()


def device_tables(H: int, W: int, R: int, device) -> dict:
    """resize_tables on `device`, in the form ops.frames_to_patches takes ("stage_rows": a per-P cache on the host)."""
    t = resize_tables(H, W, R)
    d = {k: torch.from_numpy(t[k]).to(device).contiguous() for k in ("hx_min", "hx_len", "hx_w", "vy_min", "vy_len", "vy_w")}
    d["R"] = R

    class _Rows(dict):
        def __missing__(self, P):
            self[P] = stage_rows(t, P)
            return self[P]
    d["stage_rows"] = _Rows()
    return d


LDS_BYTES = 65536        # vct_frames_to_patches: tables + staged rows + one patch


def staging_bytes(tables: dict, P: int) -> int:
    kx, ky = tables["hx_w"].shape[1], tables["vy_w"].shape[1]
    return 4 * P * (kx + ky + 4) + (stage_rows(tables, P) * P * 3 + 15) // 16 * 16 + 3 * P * P


# ---- weights ------------------------------------------------------------------------------------------------------------------------
def _get(sd, key, shape=None, ndim=None):
    if key not in sd:
        raise ValueError(f"CLIP vision tower: key {key!r} is missing from the state dict")
    t = sd[key]
    if not torch.is_tensor(t):
        t = torch.as_tensor(t)
    if ndim is not None and t.dim() != ndim:
        raise ValueError(f"CLIP vision tower: {key!r} must have {ndim} dimensions, got shape {tuple(t.shape)}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"CLIP vision tower: {key!r} must have shape {tuple(shape)}, got {tuple(t.shape)}")
    return t.detach().to("cpu", torch.float32)        # fp16 -> fp32 is exact


def _n_layers(sd, pattern):
    idx = [int(m.group(1)) for k in sd for m in [re.match(pattern, k)] if m]
    if not idx:
        raise ValueError("CLIP vision tower: the state dict holds no Transformer layer")
    return max(idx) + 1


def canonical_vision_weights(sd: Dict[str, torch.Tensor], prefix: str = "") -> dict:
    """Either key convention -> {"conv" [W, 3 P P], "patch" P, "cls" [W], "pos" [L, W], "lnpre_g", "lnpre_b", "layers": [text.py's
    layer dict], "lnpost_g", "lnpost_b", "proj" [P_out, W] (used as x @ proj.T)}: fp32 CPU tensors.  Shapes are read from the tensors
    and checked against each other; a missing or mis-shaped key is a ValueError naming it.  prefix: stripped from the front of every
    key first ("clip." for a CLIP4Clip checkpoint); keys without it are ignored."""
    if prefix:
        sd = {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}
    hf = "vision_model.embeddings.patch_embedding.weight" in sd
    if not hf and "visual.conv1.weight" not in sd:
        raise ValueError("CLIP vision tower: neither 'visual.conv1.weight' (OpenAI CLIP's state_dict) nor "
                         "'vision_model.embeddings.patch_embedding.weight' (transformers) is in the state dict"
                         + (f" under the prefix {prefix!r}" if prefix else ""))
    if hf:
        p = "vision_model."
        conv_key, pos_key = p + "embeddings.patch_embedding.weight", p + "embeddings.position_embedding.weight"
        conv = _get(sd, conv_key, ndim=4)
        W = conv.shape[0]
        cls = _get(sd, p + "embeddings.class_embedding", (W,))
        pos = _get(sd, pos_key, ndim=2)
        lnpre = _get(sd, p + "pre_layrnorm.weight", (W,)), _get(sd, p + "pre_layrnorm.bias", (W,))
        n = _n_layers(sd, r"vision_model\.encoder\.layers\.(\d+)\.")
        layers = []
        for l in range(n):
            q = p + f"encoder.layers.{l}."
            ff = _get(sd, q + "mlp.fc1.weight", ndim=2).shape[0]
            ws = [_get(sd, q + f"self_attn.{x}_proj.weight", (W, W)) for x in "qkv"]
            bs = [_get(sd, q + f"self_attn.{x}_proj.bias", (W,)) for x in "qkv"]
            layers.append({"ln1_g": _get(sd, q + "layer_norm1.weight", (W,)), "ln1_b": _get(sd, q + "layer_norm1.bias", (W,)),
                           "w_qkv": torch.cat(ws, 0), "b_qkv": torch.cat(bs, 0),
                           "w_o": _get(sd, q + "self_attn.out_proj.weight", (W, W)), "b_o": _get(sd, q + "self_attn.out_proj.bias", (W,)),
                           "ln2_g": _get(sd, q + "layer_norm2.weight", (W,)), "ln2_b": _get(sd, q + "layer_norm2.bias", (W,)),
                           "w_fc": _get(sd, q + "mlp.fc1.weight", (ff, W)), "b_fc": _get(sd, q + "mlp.fc1.bias", (ff,)),
                           "w_proj": _get(sd, q + "mlp.fc2.weight", (W, ff)), "b_proj": _get(sd, q + "mlp.fc2.bias", (W,))})
        lnpost = _get(sd, p + "post_layernorm.weight", (W,)), _get(sd, p + "post_layernorm.bias", (W,))
        proj = _get(sd, "visual_projection.weight", ndim=2)               # [P_out, W]
        if proj.shape[1] != W:
            raise ValueError(f"CLIP vision tower: 'visual_projection.weight' must have shape [P_out, {W}], got {tuple(proj.shape)}")
    else:
        p = "visual."
        conv_key, pos_key = p + "conv1.weight", p + "positional_embedding"
        conv = _get(sd, conv_key, ndim=4)
        W = conv.shape[0]
        cls = _get(sd, p + "class_embedding", (W,))
        pos = _get(sd, pos_key, ndim=2)
        lnpre = _get(sd, p + "ln_pre.weight", (W,)), _get(sd, p + "ln_pre.bias", (W,))
        n = _n_layers(sd, r"visual\.transformer\.resblocks\.(\d+)\.")
        layers = []
        for l in range(n):
            q = p + f"transformer.resblocks.{l}."
            ff = _get(sd, q + "mlp.c_fc.weight", ndim=2).shape[0]
            layers.append({"ln1_g": _get(sd, q + "ln_1.weight", (W,)), "ln1_b": _get(sd, q + "ln_1.bias", (W,)),
                           "w_qkv": _get(sd, q + "attn.in_proj_weight", (3 * W, W)), "b_qkv": _get(sd, q + "attn.in_proj_bias", (3 * W,)),
                           "w_o": _get(sd, q + "attn.out_proj.weight", (W, W)), "b_o": _get(sd, q + "attn.out_proj.bias", (W,)),
                           "ln2_g": _get(sd, q + "ln_2.weight", (W,)), "ln2_b": _get(sd, q + "ln_2.bias", (W,)),
                           "w_fc": _get(sd, q + "mlp.c_fc.weight", (ff, W)), "b_fc": _get(sd, q + "mlp.c_fc.bias", (ff,)),
                           "w_proj": _get(sd, q + "mlp.c_proj.weight", (W, ff)), "b_proj": _get(sd, q + "mlp.c_proj.bias", (W,))})
        lnpost = _get(sd, p + "ln_post.weight", (W,)), _get(sd, p + "ln_post.bias", (W,))
        proj = _get(sd, p + "proj", ndim=2)                               # [W, P_out], used as x @ proj
        if proj.shape[0] != W:
            raise ValueError(f"CLIP vision tower: 'visual.proj' must have shape [{W}, P_out], got {tuple(proj.shape)}")
        proj = proj.t().contiguous()
    P = conv.shape[2]
    if conv.shape[1] != 3 or conv.shape[3] != P or P < 1:
        raise ValueError(f"CLIP vision tower: {conv_key!r} must have shape [{W}, 3, P, P], got {tuple(conv.shape)}")
    G = math.isqrt(max(pos.shape[0] - 1, 0))
    if pos.shape[1] != W or G < 1 or G * G + 1 != pos.shape[0]:
        raise ValueError(f"CLIP vision tower: {pos_key!r} must have shape [G * G + 1, {W}], got {tuple(pos.shape)}")
    return {"conv": conv.reshape(W, 3 * P * P).contiguous(), "patch": P, "cls": cls, "pos": pos, "lnpre_g": lnpre[0], "lnpre_b": lnpre[1],
            "layers": layers, "lnpost_g": lnpost[0], "lnpost_b": lnpost[1], "proj": proj.contiguous()}


class ClipVisionTower:
    """See the module docstring.  `dim` = P_out is what the caption model's first `modal_shape` entry must equal (evaluate.v2t_frames)."""

    def __init__(self, weights: dict, device, compute_dtype=torch.bfloat16, heads: Optional[int] = None, mean=CLIP_MEAN, std=CLIP_STD):
        if compute_dtype not in (torch.bfloat16, torch.float32):
            raise ValueError(f"CLIP vision tower: compute_dtype must be torch.bfloat16 or torch.float32, got {compute_dtype}")
        cw = weights
        self.width, self.patch = cw["conv"].shape[0], int(cw["patch"])
        self.rows = cw["pos"].shape[0]                                     # L = G * G + 1 rows per frame
        self.grid = math.isqrt(self.rows - 1)
        self.resolution = self.grid * self.patch
        self.layers, self.ff, self.dim = len(cw["layers"]), cw["layers"][0]["w_fc"].shape[0], cw["proj"].shape[0]
        self.heads = int(heads) if heads is not None else self.width // 64          # CLIP: heads = width // 64
        W, H, P = self.width, self.heads, self.patch
        if self.rows > MAX_LEN:
            raise ValueError(f"CLIP vision tower: {self.resolution} px in {P} x {P} patches is {self.rows} rows per frame; at most "
                             f"{MAX_LEN} are supported (the attention kernel's limit: ViT-B/32 at 224 px has 50, ViT-B/16 and ViT-L/14 "
                             f"do not fit)")
        if H < 1 or W % H:
            raise ValueError(f"CLIP vision tower: width {W} is not divisible into {H} heads (W % heads)")
        hd = W // H
        if hd % 8 or hd > 128 or W % 8 or W > 1024 or self.ff % 8:
            raise ValueError(f"CLIP vision tower: width {W} (multiple of 8, <= 1024), head size {hd} (multiple of 8, <= 128) and "
                             f"ff {self.ff} (multiple of 8) are what the kernels take")
        if P % 8:
            raise ValueError(f"CLIP vision tower: patch size {P} must be a multiple of 8 (vct_frames_to_patches stores 16 bytes along a "
                             f"patch row)")
        if len(mean) != 3 or len(std) != 3:
            raise ValueError("CLIP vision tower: mean and std are three values each (RGB)")
        for lw in cw["layers"]:
            if lw["w_fc"].shape[0] != self.ff:
                raise ValueError("CLIP vision tower: the layers' feed-forward widths differ")
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.compute_dtype = compute_dtype
        dev, cd = self.device, compute_dtype
        f32 = lambda t: t.to(dev, torch.float32).contiguous()          # noqa: E731
        op = lambda t: t.to(dev, torch.float32).to(cd).contiguous()    # noqa: E731  GEMM operand: rounded ONCE, here
        self.conv, self.cls, self.pos = op(cw["conv"]), f32(cw["cls"]), f32(cw["pos"])
        self.lnpre_g, self.lnpre_b = f32(cw["lnpre_g"]), f32(cw["lnpre_b"])
        self.lw = [{k: (op(lw[k]) if k.startswith("w_") else f32(lw[k])) for k in _LAYER_KEYS} for lw in cw["layers"]]
        self.lnpost_g, self.lnpost_b, self.proj = f32(cw["lnpost_g"]), f32(cw["lnpost_b"]), op(cw["proj"])
        self.mean, self.std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
        self.lut = value_table(self.mean, self.std, cd).to(dev)
        self._tables = {}
        self._bufs = {}
        self.kept = None                                                # encode_frames(keep=True): every stored intermediate

    # ---- construction ----------------------------------------------------------------------------------------------------------------
    @classmethod
    def from_state_dict(cls, sd, device, compute_dtype=torch.bfloat16, heads=None, mean=CLIP_MEAN, std=CLIP_STD, prefix=""):
        return cls(canonical_vision_weights(sd, prefix), device, compute_dtype, heads, mean, std)

    @classmethod
    def from_file(cls, path, device, compute_dtype=torch.bfloat16, heads=None, mean=CLIP_MEAN, std=CLIP_STD, prefix=""):
        sd = torch.load(path, map_location="cpu")
        if hasattr(sd, "state_dict"):
            sd = sd.state_dict()
        if not isinstance(sd, dict):
            raise ValueError(f"CLIP vision tower: {path} holds a {type(sd).__name__}, not a state dict")
        return cls.from_state_dict(sd, device, compute_dtype, heads, mean, std, prefix)

    # ---- forward ---------------------------------------------------------------------------------------------------------------------
    def tables(self, H: int, W: int) -> dict:
        """The device copy of resize_tables(H, W, R), cached; ValueError when a patch's window does not fit the staging."""
        t = self._tables.get((H, W))
        if t is None:
            host = resize_tables(H, W, self.resolution)
            need = staging_bytes(host, self.patch)
            if need > LDS_BYTES:
                raise ValueError(f"CLIP vision tower: {H} x {W} frames need {need} bytes of staging per patch ({stage_rows(host, self.patch)} "
                                 f"input rows), over the {LDS_BYTES} bytes of vct_frames_to_patches; downscale the frames first")
            t = self._tables[(H, W)] = device_tables(H, W, self.resolution, self.device)
        return t

    def _buffers(self, N):
        b = self._bufs.get(N)
        if b is None:
            dev, cd, W, L, P = self.device, self.compute_dtype, self.width, self.rows, self.patch
            M = N * L
            b = self._bufs[N] = {
                "a": torch.empty(N * (L - 1), 3 * P * P, dtype=cd, device=dev), "e": torch.empty(N * (L - 1), W, dtype=torch.float32, device=dev),
                "xa": torch.empty(M, W, dtype=torch.float32, device=dev), "xb": torch.empty(M, W, dtype=torch.float32, device=dev),
                "h": torch.empty(M, W, dtype=cd, device=dev), "qkv": torch.empty(M, 3 * W, dtype=cd, device=dev),
                "o": torch.empty(M, W, dtype=cd, device=dev), "f": torch.empty(M, self.ff, dtype=cd, device=dev),
                "pooled": torch.empty(N, W, dtype=cd, device=dev)}
        return b

    def _check_frames(self, frames):
        if not torch.is_tensor(frames) or frames.dim() != 4 or frames.dtype != torch.uint8 or frames.shape[3] != 3 \
                or min(frames.shape[:3]) < 1:
            got = (tuple(frames.shape), frames.dtype) if torch.is_tensor(frames) else type(frames)
            raise ValueError(f"CLIP vision tower: frames must be a uint8 [N, H, W, 3] tensor (RGB), got {got}")

    @torch.no_grad()
    def encode_frames(self, frames: torch.Tensor, out: Optional[torch.Tensor] = None, keep: bool = False) -> torch.Tensor:
        """frames: uint8 [N, H, W, 3] (RGB), on the host or this device -> fp32 [N, P_out] on the device (a new tensor, or `out`).
        keep: clones of every stored intermediate (and the cropped uint8 image) are left in self.kept (tests)."""
        self._check_frames(frames)
        N, H, W_in, _ = frames.shape
        tables = self.tables(H, W_in)
        if frames.device.type == "cpu":
            frames = frames.contiguous().to(self.device, non_blocking=True)
        elif frames.device != self.device:
            raise ValueError(f"CLIP vision tower: frames are on {frames.device}, the tower is on {self.device}")
        else:
            frames = frames.contiguous()
        if out is None:
            out = torch.empty(N, self.dim, dtype=torch.float32, device=self.device)
        elif out.dtype != torch.float32 or tuple(out.shape) != (N, self.dim) or out.device != self.device or out.stride(1) != 1:
            raise ValueError(f"CLIP vision tower: out must be fp32 [{N}, {self.dim}] on {self.device}")
        b = self._buffers(N)
        xa, R = b["xa"], self.resolution
        kept = {"layers": []} if keep else None
        crop = torch.empty(N, R, R, 3, dtype=torch.uint8, device=self.device) if keep else None
        ops.frames_to_patches(frames, tables, self.lut, self.patch, b["a"], crop)
        ops.gemm(b["a"], self.conv, b["e"])
        ops.vit_embed(b["e"], self.cls, self.pos, self.lnpre_g, self.lnpre_b, xa)
        if keep:
            kept.update(crop=crop, a=b["a"].clone(), e=b["e"].clone(), x0=xa.clone())
        run_layers(self.lw, xa, b["xb"], b["h"], b["qkv"], b["o"], b["f"], N, self.heads, self.rows, False,
                   kept["layers"] if keep else None)
        ops.vit_pool(xa, self.rows, self.lnpost_g, self.lnpost_b, b["pooled"])
        ops.gemm(b["pooled"], self.proj, out)
        if keep:
            kept.update(pooled=b["pooled"].clone(), out=out.clone())
            self.kept = kept
        return out

    __call__ = encode_frames

    @torch.no_grad()
    def encode_all(self, frames: torch.Tensor, chunk: int = 256, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Many frames of one size: uint8 [N, H, W, 3] -> fp32 [N, P_out], chunk by chunk into ONE matrix (`out`, or a new one)."""
        self._check_frames(frames)
        N = frames.shape[0]
        if chunk < 1:
            raise ValueError("CLIP vision tower: chunk must be at least 1")
        if out is None:
            out = torch.empty(N, self.dim, dtype=torch.float32, device=self.device)
        elif out.dtype != torch.float32 or tuple(out.shape) != (N, self.dim) or out.device != self.device or not out.is_contiguous():
            raise ValueError(f"CLIP vision tower: out must be a contiguous fp32 [{N}, {self.dim}] on {self.device}")
        for i in range(0, N, chunk):
            self.encode_frames(frames[i:i + chunk], out=out[i:i + chunk])
        return out
