"""Writes tests/golden/text_tower.npz: a small transformers.CLIPTextModelWithProjection (width 64, 4 heads, ff 256, 3 layers,
projection 48, vocabulary 300, quick_gelu), five captions and the module's own fp64 outputs -- so that the GPU tests need neither
`transformers` nor a tokenizer.  CPU only; run it where `transformers` imports:

    python tools/make_golden_text_tower.py

Size.  The model has 175 k parameters: 700 KB in fp32.  Every tensor is therefore drawn on an int8 grid (value = q * 2^-k, one k per
tensor, |q| <= 127) and stored as int8 plus its scale -- 180 KB.  The module computes its outputs FROM those grid values, so nothing is
lost by the storage, and the values are exact in fp16 and bf16 as well (rounding the weights at load is the identity for this model;
tests of the rounding points use tests/text_tower_ref.random_state_dict instead).
Keys: `q/<state-dict key>` int8, `scale/<key>` fp64 scalar (transformers' key convention), `ids` int64 [5, 77] (EOT = 299 at index
3 / 9 / 20 / 63 / 12, start token 298), `eot` int64 [5], `out` fp64 [5, 48] = text_embeds at 77 positions, `heads`."""
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPE = dict(vocab_size=300, hidden_size=64, intermediate_size=256, num_hidden_layers=3, num_attention_heads=4,
             max_position_embeddings=77, projection_dim=48)
EOTS = (3, 9, 20, 63, 12)


def grid(t):
    """t -> (q int8, scale): the nearest values q * 2^-k with |q| <= 127."""
    k = math.floor(math.log2(127.0 / float(t.abs().max())))
    s = 2.0 ** -k
    return torch.clamp(torch.round(t / s), -127, 127).to(torch.int8), s


def main():
    from transformers import CLIPTextConfig, CLIPTextModelWithProjection
    import text_tower_ref as R
    torch.manual_seed(20)
    cfg = CLIPTextConfig(hidden_act="quick_gelu", eos_token_id=2, bos_token_id=0, pad_token_id=1, **SHAPE)
    m = CLIPTextModelWithProjection(cfg).double().eval()
    sd = m.state_dict()
    g = torch.Generator().manual_seed(21)
    stored, new = {}, {}
    for k, v in sd.items():
        if not v.is_floating_point():
            continue
        if "embedding" in k:
            t = torch.randn(v.shape, generator=g, dtype=torch.float64) * (0.5 if "token" in k else 0.3)
        elif "layer_norm" in k and k.endswith("weight"):
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
    ids = R.caption_ids(EOTS, SHAPE["vocab_size"], seed=22)
    with torch.no_grad():
        out = m(input_ids=ids).text_embeds
    mine = R.tower(new, ids, SHAPE["num_attention_heads"])
    err = float((mine - out).abs().max() / out.abs().max())
    assert err < 1e-12, err
    path = os.path.join(ROOT, "tests", "golden", "text_tower.npz")
    np.savez_compressed(path, ids=ids.numpy(), eot=np.asarray(EOTS, np.int64), out=out.numpy(),
                        heads=np.int64(SHAPE["num_attention_heads"]), **stored)
    print(f"{path}: {os.path.getsize(path)} bytes; restatement vs transformers {err:.2e}")


if __name__ == "__main__":
    main()
