"""Writes tests/golden/vision_tower.npz: a small transformers.CLIPVisionModelWithProjection (width 64, 2 heads, ff 128, 3 layers, 16 x 16
patches of a 32 px image, projection 48, quick_gelu), two uint8 frames of 40 x 56 and the module's own fp64 outputs on CLIP's
preprocessing of them -- so that the GPU tests need neither `transformers` nor PIL.  CPU only; run it where `transformers` imports:

    python tools/make_golden_vision_tower.py

Size.  The model has 150 k parameters.  As in tools/make_golden_text_tower.py every tensor is drawn on an int8 grid (value = q * 2^-k,
one k per tensor, |q| <= 127) and stored as int8 plus its scale; the module computes its outputs FROM those grid values, which are
exact in fp16 and bf16 as well.
Keys: `q/<state-dict key>` int8, `scale/<key>` fp64 scalar (transformers' key convention), `frames` uint8 [2, 40, 56, 3], `crop` uint8
[2, 32, 32, 3] (PIL's resize + centre crop), `out` fp64 [2, 48] = image_embeds, `heads`."""
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPE = dict(hidden_size=64, intermediate_size=128, num_hidden_layers=3, num_attention_heads=2, image_size=32, patch_size=16,
             projection_dim=48)


def grid(t):
    """t -> (q int8, scale): the nearest values q * 2^-k with |q| <= 127."""
    k = math.floor(math.log2(127.0 / float(t.abs().max())))
    s = 2.0 ** -k
    return torch.clamp(torch.round(t / s), -127, 127).to(torch.int8), s


def main():
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
    import vision_ref as R
    torch.manual_seed(30)
    m = CLIPVisionModelWithProjection(CLIPVisionConfig(hidden_act="quick_gelu", **SHAPE)).double().eval()
    g = torch.Generator().manual_seed(31)
    stored, new = {}, {}
    for k, v in m.state_dict().items():
        if not v.is_floating_point():
            continue
        if "patch_embedding" in k:
            t = torch.randn(v.shape, generator=g, dtype=torch.float64) * (3 * 16 * 16) ** -0.5
        elif "embedding" in k:
            t = torch.randn(v.shape, generator=g, dtype=torch.float64) * (0.5 if "class" in k else 0.3)
        elif ("layer_norm" in k or "layrnorm" in k or "layernorm" in k) and k.endswith("weight"):
            t = 1.0 + 0.1 * torch.randn(v.shape, generator=g, dtype=torch.float64)
        elif k.endswith("bias"):
            t = 0.1 * torch.randn(v.shape, generator=g, dtype=torch.float64)
        else:
            t = 0.08 * torch.randn(v.shape, generator=g, dtype=torch.float64)
        q, s = grid(t)
        stored["q/" + k], stored["scale/" + k] = q.numpy(), np.float64(s)
        new[k] = q.to(torch.float64) * s
    missing = m.load_state_dict(new, strict=False)
    assert not missing.unexpected_keys and all("position_ids" in k for k in missing.missing_keys), missing
    frames = R.random_frames(2, 40, 56, seed=32)
    crop = np.stack([R.pil_preprocess_u8(f, 32) for f in frames])
    lut = R.value_table()
    pixels = torch.stack([lut[c][torch.from_numpy(crop[..., c]).long()] for c in range(3)], 1).double()       # [N, 3, R, R]
    with torch.no_grad():
        out = m(pixel_values=pixels).image_embeds
    mine = R.tower(new, frames, SHAPE["num_attention_heads"])
    err = float((mine - out).abs().max() / out.abs().max())
    assert err < 1e-12, err
    path = os.path.join(ROOT, "tests", "golden", "vision_tower.npz")
    np.savez_compressed(path, frames=frames, crop=crop, out=out.numpy(), heads=np.int64(SHAPE["num_attention_heads"]), **stored)
    print(f"{path}: {os.path.getsize(path)} bytes; restatement vs transformers {err:.2e}")


if __name__ == "__main__":
    main()
