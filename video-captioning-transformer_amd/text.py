"""A frozen, forward-only CLIP text tower on the library's kernels: ids -> fp32 [B, P] sentence features.

The definition is OpenAI CLIP's `encode_text` (clip/model.py), which the reference reaches from model/TextEncoder.py:

    x = token_embedding[ids] + positional_embedding[:L]
    per layer:  x = x + out_proj(MHA(ln_1(x), causal));  x = x + c_proj(QuickGELU(c_fc(ln_2(x))))
    y = ln_final(x)[b, e_b] @ text_projection,   e_b = FIRST index of the maximum of ids[b] (the EOT token has the largest id)

The mask is causal, so no position behind e_b can reach row e_b: running the first L = max_b e_b + 1 positions is exact.  The ids come
from a host tokenizer, so L is a host decision; L > 64 (the attention kernel's limit) is refused, never truncated.

Schedule, seven launches per layer and three around them:
    vct_embed_fwd (fp32 stream) | vct_preln_fwd, vct_gemm [3W, W] + bias, vct_attn_fwd causal, vct_gemm out_proj + bias + stream -> fp32,
    vct_preln_fwd, vct_gemm c_fc + bias + QuickGELU, vct_gemm c_proj + bias + stream -> fp32 | vct_text_pool, vct_gemm projection -> fp32
The per-layer launches are run_layers, which the vision tower (vision.py) shares.  The residual stream is fp32 in both modes; the GEMM operands are bf16 (rounded once, at load) or fp32 (parity mode).  Everything is
enqueued on the current stream through the runtime's launch wrapper; nothing synchronises.  The weights are no part of any
state_dict (the reference's TextEncoder is not a module either).  No tokenizer is shipped: CLIP's BPE merges are a download -- pass
`tokenize=clip.tokenize` (or an equivalent strings -> int [B, 77] callable), or pass ids."""
import re
from typing import Callable, Dict, Optional

import torch

from . import ops

CONTEXT = 77        # CLIP's context length
MAX_LEN = 64        # vct_attn_fwd: Lq, Lk <= 64

_LAYER_KEYS = ("ln1_g", "ln1_b", "w_qkv", "b_qkv", "w_o", "b_o", "ln2_g", "ln2_b", "w_fc", "b_fc", "w_proj", "b_proj")


def _get(sd, key, shape=None, ndim=None):
    if key not in sd:
        raise ValueError(f"CLIP text tower: key {key!r} is missing from the state dict")
    t = sd[key]
    if not torch.is_tensor(t):
        t = torch.as_tensor(t)
    if ndim is not None and t.dim() != ndim:
        raise ValueError(f"CLIP text tower: {key!r} must have {ndim} dimensions, got shape {tuple(t.shape)}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"CLIP text tower: {key!r} must have shape {tuple(shape)}, got {tuple(t.shape)}")
    return t.detach().to("cpu", torch.float32)        # fp16 -> fp32 is exact


def _n_layers(sd, pattern):
    idx = [int(m.group(1)) for k in sd for m in [re.match(pattern, k)] if m]
    if not idx:
        raise ValueError("CLIP text tower: the state dict holds no Transformer layer")
    return max(idx) + 1


def canonical_weights(sd: Dict[str, torch.Tensor]) -> dict:
    """Either key convention -> {"tok" [V, W], "pos" [77, W], "layers": [{ln1_g, ln1_b, w_qkv [3W, W], b_qkv, w_o, b_o, ln2_g, ln2_b,
    w_fc [ff, W], b_fc, w_proj [W, ff], b_proj}], "lnf_g", "lnf_b", "proj" [P, W] (used as x @ proj.T)}: fp32 CPU tensors.
    Shapes are read from the tensors and checked against each other; a missing or mis-shaped key is a ValueError naming it."""
    hf = "text_model.embeddings.token_embedding.weight" in sd
    if not hf and "token_embedding.weight" not in sd:
        raise ValueError("CLIP text tower: neither 'token_embedding.weight' (OpenAI CLIP's state_dict) nor "
                         "'text_model.embeddings.token_embedding.weight' (transformers) is in the state dict")
    if hf:
        p = "text_model."
        tok = _get(sd, p + "embeddings.token_embedding.weight", ndim=2)
        W = tok.shape[1]
        pos = _get(sd, p + "embeddings.position_embedding.weight", ndim=2)
        n = _n_layers(sd, r"text_model\.encoder\.layers\.(\d+)\.")
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
        lnf_g, lnf_b = _get(sd, p + "final_layer_norm.weight", (W,)), _get(sd, p + "final_layer_norm.bias", (W,))
        proj = _get(sd, "text_projection.weight", ndim=2)                 # [P, W]
        if proj.shape[1] != W:
            raise ValueError(f"CLIP text tower: 'text_projection.weight' must have shape [P, {W}], got {tuple(proj.shape)}")
    else:
        tok = _get(sd, "token_embedding.weight", ndim=2)
        W = tok.shape[1]
        pos = _get(sd, "positional_embedding", ndim=2)
        n = _n_layers(sd, r"transformer\.resblocks\.(\d+)\.")
        layers = []
        for l in range(n):
            q = f"transformer.resblocks.{l}."
            ff = _get(sd, q + "mlp.c_fc.weight", ndim=2).shape[0]
            layers.append({"ln1_g": _get(sd, q + "ln_1.weight", (W,)), "ln1_b": _get(sd, q + "ln_1.bias", (W,)),
                           "w_qkv": _get(sd, q + "attn.in_proj_weight", (3 * W, W)), "b_qkv": _get(sd, q + "attn.in_proj_bias", (3 * W,)),
                           "w_o": _get(sd, q + "attn.out_proj.weight", (W, W)), "b_o": _get(sd, q + "attn.out_proj.bias", (W,)),
                           "ln2_g": _get(sd, q + "ln_2.weight", (W,)), "ln2_b": _get(sd, q + "ln_2.bias", (W,)),
                           "w_fc": _get(sd, q + "mlp.c_fc.weight", (ff, W)), "b_fc": _get(sd, q + "mlp.c_fc.bias", (ff,)),
                           "w_proj": _get(sd, q + "mlp.c_proj.weight", (W, ff)), "b_proj": _get(sd, q + "mlp.c_proj.bias", (W,))})
        lnf_g, lnf_b = _get(sd, "ln_final.weight", (W,)), _get(sd, "ln_final.bias", (W,))
        proj = _get(sd, "text_projection", ndim=2)                        # [W, P], used as x @ P
        if proj.shape[0] != W:
            raise ValueError(f"CLIP text tower: 'text_projection' must have shape [{W}, P], got {tuple(proj.shape)}")
        proj = proj.t().contiguous()
    pos_key = "text_model.embeddings.position_embedding.weight" if hf else "positional_embedding"
    if pos.shape[1] != W or pos.shape[0] < 1:
        raise ValueError(f"CLIP text tower: {pos_key!r} must have shape [positions, {W}], got {tuple(pos.shape)}")
    return {"tok": tok, "pos": pos, "layers": layers, "lnf_g": lnf_g, "lnf_b": lnf_b, "proj": proj.contiguous()}


def to_openai_keys(cw: dict) -> Dict[str, torch.Tensor]:
    """canonical_weights' form -> OpenAI CLIP's state_dict keys (text tower only)."""
    sd = {"token_embedding.weight": cw["tok"], "positional_embedding": cw["pos"], "ln_final.weight": cw["lnf_g"],
          "ln_final.bias": cw["lnf_b"], "text_projection": cw["proj"].t().contiguous()}
    names = {"ln1_g": "ln_1.weight", "ln1_b": "ln_1.bias", "w_qkv": "attn.in_proj_weight", "b_qkv": "attn.in_proj_bias",
             "w_o": "attn.out_proj.weight", "b_o": "attn.out_proj.bias", "ln2_g": "ln_2.weight", "ln2_b": "ln_2.bias",
             "w_fc": "mlp.c_fc.weight", "b_fc": "mlp.c_fc.bias", "w_proj": "mlp.c_proj.weight", "b_proj": "mlp.c_proj.bias"}
    for l, lw in enumerate(cw["layers"]):
        for k, name in names.items():
            sd[f"transformer.resblocks.{l}.{name}"] = lw[k]
    return sd


def to_transformers_keys(cw: dict) -> Dict[str, torch.Tensor]:
    """canonical_weights' form -> the keys of transformers.CLIPTextModelWithProjection."""
    p = "text_model."
    sd = {p + "embeddings.token_embedding.weight": cw["tok"], p + "embeddings.position_embedding.weight": cw["pos"],
          p + "final_layer_norm.weight": cw["lnf_g"], p + "final_layer_norm.bias": cw["lnf_b"], "text_projection.weight": cw["proj"]}
    for l, lw in enumerate(cw["layers"]):
        q = p + f"encoder.layers.{l}."
        W = lw["w_o"].shape[0]
        for i, x in enumerate("qkv"):
            sd[q + f"self_attn.{x}_proj.weight"] = lw["w_qkv"][i * W:(i + 1) * W].contiguous()
            sd[q + f"self_attn.{x}_proj.bias"] = lw["b_qkv"][i * W:(i + 1) * W].contiguous()
        sd[q + "self_attn.out_proj.weight"], sd[q + "self_attn.out_proj.bias"] = lw["w_o"], lw["b_o"]
        sd[q + "layer_norm1.weight"], sd[q + "layer_norm1.bias"] = lw["ln1_g"], lw["ln1_b"]
        sd[q + "layer_norm2.weight"], sd[q + "layer_norm2.bias"] = lw["ln2_g"], lw["ln2_b"]
        sd[q + "mlp.fc1.weight"], sd[q + "mlp.fc1.bias"] = lw["w_fc"], lw["b_fc"]
        sd[q + "mlp.fc2.weight"], sd[q + "mlp.fc2.bias"] = lw["w_proj"], lw["b_proj"]
    return sd


def eot_positions(ids: torch.Tensor) -> torch.Tensor:
    """First index of each row's maximum (int64 [B]): torch.argmax documents no tie rule, CLIP's EOT rule needs the first."""
    ids = ids.to(torch.int64)
    n = ids.shape[1]
    is_max = ids == ids.max(dim=1, keepdim=True).values
    cols = torch.arange(n, dtype=torch.int64, device=ids.device).expand_as(ids)
    return torch.where(is_max, cols, torch.full_like(cols, n)).min(dim=1).values


def trim_length(ids: torch.Tensor) -> int:
    """Host ids -> L = max_b e_b + 1; ValueError when that is over MAX_LEN (names the limit and the first offending caption)."""
    e = eot_positions(ids)
    L = int(e.max()) + 1
    if L > MAX_LEN:
        bad = int((e >= MAX_LEN).nonzero()[0])
        raise ValueError(f"CLIP text tower: caption {bad} has its end-of-text token at position {int(e[bad])}, i.e. {int(e[bad]) + 1} "
                         f"tokens; at most {MAX_LEN} positions are supported (the attention kernel's limit) and captions are never "
                         f"truncated silently")
    return L


def run_layers(lws, xa, xb, h, qkv, o, f, B, H, L, causal, kept=None):
    """CLIP's pre-LN ResidualAttentionBlock over the fp32 stream xa [B * L, W], seven launches per layer; the result is in xa again.
    xb: the second stream buffer; h, qkv, o, f: compute-dtype scratch [B * L, W | 3 W | W | ff].  kept: a list that receives clones of
    every stored intermediate, one dict per layer.  Shared by the text tower (causal) and the vision tower (vision.py; not causal)."""
    W = xa.shape[1]
    for lw in lws:
        ops.preln_fwd(xa, lw["ln1_g"], lw["ln1_b"], h)
        if kept is not None:
            k = {"h1": h.clone()}
        ops.gemm(h, lw["w_qkv"], qkv, bias=lw["b_qkv"])
        ops.attn_fwd(qkv[:, :W], qkv[:, W:2 * W], qkv[:, 2 * W:], o, B, H, L, L, causal=causal)
        ops.gemm(o, lw["w_o"], xb, bias=lw["b_o"], addend=xa)
        ops.preln_fwd(xb, lw["ln2_g"], lw["ln2_b"], h)
        if kept is not None:
            k.update(qkv=qkv.clone(), o=o.clone(), x1=xb.clone(), h2=h.clone())
        ops.gemm(h, lw["w_fc"], f, bias=lw["b_fc"], act="quick_gelu")
        ops.gemm(f, lw["w_proj"], xa, bias=lw["b_proj"], addend=xb)
        if kept is not None:
            k.update(f=f.clone(), x2=xa.clone())
            kept.append(k)


class ClipTextTower:
    """See the module docstring. `dim` = P is what Matching / TextEncoder.dim must equal."""

    def __init__(self, weights: dict, device, compute_dtype=torch.bfloat16, tokenize: Optional[Callable] = None,
                 heads: Optional[int] = None):
        if compute_dtype not in (torch.bfloat16, torch.float32):
            raise ValueError(f"CLIP text tower: compute_dtype must be torch.bfloat16 or torch.float32, got {compute_dtype}")
        cw = weights
        self.vocab, self.width = cw["tok"].shape
        self.layers, self.ff, self.dim = len(cw["layers"]), cw["layers"][0]["w_fc"].shape[0], cw["proj"].shape[0]
        self.positions = cw["pos"].shape[0]
        self.heads = int(heads) if heads is not None else self.width // 64          # CLIP: heads = width // 64
        W, H = self.width, self.heads
        if H < 1 or W % H:
            raise ValueError(f"CLIP text tower: width {W} is not divisible into {H} heads (W % heads)")
        hd = W // H
        if hd % 8 or hd > 128 or W % 8 or W > 1024 or self.ff % 8:
            raise ValueError(f"CLIP text tower: width {W} (multiple of 8, <= 1024), head size {hd} (multiple of 8, <= 128) and "
                             f"ff {self.ff} (multiple of 8) are what the kernels take")
        for lw in cw["layers"]:
            if lw["w_fc"].shape[0] != self.ff:
                raise ValueError("CLIP text tower: the layers' feed-forward widths differ")
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.compute_dtype = compute_dtype
        self.tokenize = tokenize
        dev, cd = self.device, compute_dtype
        f32 = lambda t: t.to(dev, torch.float32).contiguous()          # noqa: E731
        op = lambda t: t.to(dev, torch.float32).to(cd).contiguous()    # noqa: E731  GEMM operand: rounded ONCE, here
        self.tok, self.pos = f32(cw["tok"]), f32(cw["pos"])
        self.lw = [{k: (op(lw[k]) if k.startswith("w_") else f32(lw[k])) for k in _LAYER_KEYS} for lw in cw["layers"]]
        self.lnf_g, self.lnf_b, self.proj = f32(cw["lnf_g"]), f32(cw["lnf_b"]), op(cw["proj"])
        self.err = torch.zeros(1, dtype=torch.int32, device=dev)        # raised by vct_text_pool, read by check()
        self._bufs = {}
        self.kept = None                                                # encode_ids(keep=True): every stored intermediate

    # ---- construction ----------------------------------------------------------------------------------------------------------------
    @classmethod
    def from_state_dict(cls, sd, device, compute_dtype=torch.bfloat16, tokenize=None, heads=None):
        return cls(canonical_weights(sd), device, compute_dtype, tokenize, heads)

    @classmethod
    def from_file(cls, path, device, compute_dtype=torch.bfloat16, tokenize=None, heads=None):
        sd = torch.load(path, map_location="cpu")
        if hasattr(sd, "state_dict"):
            sd = sd.state_dict()
        if not isinstance(sd, dict):
            raise ValueError(f"CLIP text tower: {path} holds a {type(sd).__name__}, not a state dict")
        return cls.from_state_dict(sd, device, compute_dtype, tokenize, heads)

    # ---- forward ---------------------------------------------------------------------------------------------------------------------
    def _buffers(self, B, L):
        b = self._bufs.get((B, L))
        if b is None:
            dev, cd, W, M = self.device, self.compute_dtype, self.width, B * L
            b = self._bufs[(B, L)] = {
                "xa": torch.empty(M, W, dtype=torch.float32, device=dev), "xb": torch.empty(M, W, dtype=torch.float32, device=dev),
                "h": torch.empty(M, W, dtype=cd, device=dev), "qkv": torch.empty(M, 3 * W, dtype=cd, device=dev),
                "o": torch.empty(M, W, dtype=cd, device=dev), "f": torch.empty(M, self.ff, dtype=cd, device=dev),
                "pooled": torch.empty(B, W, dtype=cd, device=dev), "eot": torch.empty(B, dtype=torch.int32, device=dev)}
        return b

    def _check_ids(self, ids):
        if not torch.is_tensor(ids) or ids.dim() != 2 or ids.dtype not in (torch.int32, torch.int64) or ids.shape[0] < 1 \
                or not 1 <= ids.shape[1] <= self.positions:
            got = (tuple(ids.shape), ids.dtype) if torch.is_tensor(ids) else type(ids)
            raise ValueError(f"CLIP text tower: ids must be an int32 / int64 [B, <= {self.positions}] tensor, got {got}")

    @torch.no_grad()
    def encode_ids(self, ids: torch.Tensor, out: Optional[torch.Tensor] = None, keep: bool = False) -> torch.Tensor:
        """ids: int32 / int64 [B, <= 77], on the host or the device -> fp32 [B, P] on the device (a new tensor, or `out`).
        Host ids are trimmed to L = max_b e_b + 1 here (ValueError over 64).  Device ids are not read back: all their columns (at
        most the first 64) are run, and a caption whose EOT lies behind them raises the device flag that check() reads.
        keep: clones of every stored intermediate are left in self.kept (tests)."""
        self._check_ids(ids)
        B = ids.shape[0]
        if ids.device.type == "cpu":
            L = trim_length(ids)
            ids_dev = ids[:, :L].to(torch.int64).contiguous().to(self.device, non_blocking=True)
        else:
            if ids.device != self.device:
                raise ValueError(f"CLIP text tower: ids are on {ids.device}, the tower is on {self.device}")
            L = min(ids.shape[1], MAX_LEN)
            ids_dev = ids.to(torch.int64).contiguous()
        if out is None:
            out = torch.empty(B, self.dim, dtype=torch.float32, device=self.device)
        elif out.dtype != torch.float32 or tuple(out.shape) != (B, self.dim) or out.device != self.device or out.stride(1) != 1:
            raise ValueError(f"CLIP text tower: out must be fp32 [{B}, {self.dim}] on {self.device}")
        b = self._buffers(B, L)
        xa, xb, h, qkv, o, f = b["xa"], b["xb"], b["h"], b["qkv"], b["o"], b["f"]
        kept = {"ids": ids_dev.clone(), "L": L, "layers": []} if keep else None
        ops.embed_fwd(ids_dev, L, self.tok, self.pos, xa)
        if keep:
            kept["x0"] = xa.clone()
        run_layers(self.lw, xa, xb, h, qkv, o, f, B, self.heads, L, True, kept["layers"] if keep else None)
        ops.text_pool(ids_dev, xa, L, self.lnf_g, self.lnf_b, b["pooled"], b["eot"], self.err)
        ops.gemm(b["pooled"], self.proj, out)
        if keep:
            kept.update(pooled=b["pooled"].clone(), eot=b["eot"].clone(), out=out.clone())
            self.kept = kept
        return out

    def __call__(self, captions) -> torch.Tensor:
        if self.tokenize is None:
            if torch.is_tensor(captions):
                return self.encode_ids(captions)
            raise RuntimeError("CLIP text tower: no tokenizer was given, so captions must be token ids (an int [B, <= 77] tensor).  No "
                               "BPE tokenizer is shipped (its merges file is a download): pass tokenize=clip.tokenize or an "
                               "equivalent to from_state_dict / from_file, or set tower.tokenize")
        return self.encode_ids(torch.as_tensor(self.tokenize(captions)))

    @torch.no_grad()
    def encode_all(self, ids: torch.Tensor, chunk: int = 1024, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """A whole split: ids [N, <= 77] -> fp32 [N, P], chunk by chunk into ONE matrix (`out`, or a new one): each chunk is trimmed
        to its own L and its rows are written in place, so the matrix is what the retrieval scorer reads."""
        self._check_ids(ids)
        N = ids.shape[0]
        if chunk < 1:
            raise ValueError("CLIP text tower: chunk must be at least 1")
        if out is None:
            out = torch.empty(N, self.dim, dtype=torch.float32, device=self.device)
        elif out.dtype != torch.float32 or tuple(out.shape) != (N, self.dim) or out.device != self.device or not out.is_contiguous():
            raise ValueError(f"CLIP text tower: out must be a contiguous fp32 [{N}, {self.dim}] on {self.device}")
        for i in range(0, N, chunk):
            self.encode_ids(ids[i:i + chunk], out=out[i:i + chunk])
        return out

    def check(self):
        """Reads the device error flag (ONE synchronisation; call it when convenient, e.g. once per epoch): a caption's EOT lay
        behind the positions that were run -- possible only for device-resident ids, host ids are trimmed and refused before."""
        if int(self.err.item()) != 0:
            self.err.zero_()
            raise ValueError(f"CLIP text tower: a caption's end-of-text token lay behind position {MAX_LEN} (or behind the ids' last "
                             f"column); its feature row is zero.  At most {MAX_LEN} positions are supported")
