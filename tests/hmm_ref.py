"""Shared by the hierarchical-encoder tests and tools/make_golden_hmm_encoder.py: the config block (`video_encoder.type: "hmme"`, one
depth per feature stream) and the deterministic parameters of such a model (the fixtures record only the seed)."""
import numpy as np

import vct_oracle as O
from encvar_ref import encvar_config, encvar_params

OLD, NEW = O.ENC + "transformer_encoder.layers.", O.ENC + "trans_enc_layers."


def hmm_config(shapes, layers, aggregation="avg", temporal="encoding", do_norm=False, **kw):
    """encvar_config with video_encoder.type 'hmme' and video_encoder.layer = the per-stream list of depths."""
    mc = encvar_config(shapes, aggregation, temporal, do_norm, **kw)
    mc["video_encoder"].update(type="hmme", layer=list(layers))
    return mc


def hmm_params(mc, vocab, seed):
    """encvar_params of the `mme` model with max(layer) layers, the layer keys renamed to trans_enc_layers.{l}.* and the stack-final
    norm dropped.  Layer l > 0 = layer 0 scaled by 1 + 0.1 l / 0.02 l N(0, 1) per element (its own generator): the oracle's
    parameters may or may not differ per layer, these do, so a row routed through the wrong layer shows."""
    L = max(mc["video_encoder"]["layer"])
    flat = dict(mc, video_encoder=dict(mc["video_encoder"], layer=L, type="mme"))
    p = encvar_params(flat, vocab, seed)
    out = {}
    for k, v in p.items():
        if k.startswith(O.ENC + "transformer_encoder.norm."):
            continue
        out[NEW + k[len(OLD):] if k.startswith(OLD) else k] = v
    rng = np.random.default_rng(seed + 3000)
    for l in range(1, L):
        for k in sorted(q for q in out if q.startswith(f"{NEW}{l}.")):
            v = out[k]
            out[k] = (v * (1.0 + 0.1 * l) + 0.02 * l * rng.standard_normal(v.shape)).astype(np.float32)
    return out


def take_table(layers, Ts):
    """The reference's routing rule restated (model/MMEncoder.py:385-396): layer i reads the previous output on the rows of stream j
    when target[j] = max(layers) - layers[j] < i."""
    L = max(layers)
    rows = []
    for i in range(L):
        rows.append(np.concatenate([np.full(t + 1, int(L - n < i), np.uint8) for n, t in zip(layers, Ts)]))
    return np.stack(rows)
