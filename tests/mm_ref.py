"""Shared by the multi-modal tests and tools/make_golden_multimodal.py: deterministic parameters of a model with n >= 1 feature
streams (the fixtures record only the seed), and the model config block."""
import math

import numpy as np

import vct_oracle as O


def mm_config(d, shapes, H, ff, Le, Ld, modal_different=True, alpha=0.5, act="gelu", dropout=0.0):
    """cfg['model'] of the reference with one entry of modal_shape per feature stream."""
    return {"modal": [f"m{i}" for i in range(len(shapes))], "modal_shape": list(shapes), "tokenizer": "stub",
            "text_enc_type": "CLIP", "embed_dim": d, "dropout": dropout, "loss_beta": 0.5,
            "matching": {"enable_tem": False, "matching_loss": "CSL"}, "activation": act,
            "video_encoder": {"layer": Le, "nhead": H, "feedforward": ff,
                              "mme": {"temporal": "encoding", "modal_different": bool(modal_different), "do_norm": False,
                                      "aggregation": "avg"}},
            "caption_decoder": {"layer": Ld, "nhead": H, "feedforward": ff, "sce_loss_alpha": alpha},
            "pretrained_model": None}


def mm_params(mc, vocab, seed):
    """The oracle's single-stream parameters (modality 0) plus unify.i (i >= 1, nn.Linear-like uniform) and the modal embedding
    (N(0, 1), nn.Embedding's init): numpy dict keyed like the reference's state_dict."""
    shapes = mc["modal_shape"]
    single = dict(mc, modal_shape=[shapes[0]])
    p = O.init_params(O.cfg_from_model_config(single, vocab), seed)
    rng = np.random.default_rng(seed + 1000)
    d = mc["embed_dim"]
    for i in range(1, len(shapes)):
        b = 1.0 / math.sqrt(shapes[i])
        p[f"{O.ENC}unify.{i}.weight"] = rng.uniform(-b, b, (d, shapes[i])).astype(np.float32)
        p[f"{O.ENC}unify.{i}.bias"] = rng.uniform(-b, b, (d,)).astype(np.float32)
    if len(shapes) > 1:
        rows = 2 * len(shapes) if mc["video_encoder"]["mme"].get("modal_different", True) else len(shapes)
        p[f"{O.ENC}modal_emb.modal_emb.weight"] = rng.standard_normal((rows, d)).astype(np.float32)
    return p


def mm_batch(B, Ts, shapes, S, vocab, seed, valid=None):
    """Per-modality features [B, T_i, E_i] and masks [B, T_i] (valid[i][b] = real frames of video b in modality i; valid None or
    valid[i] None = no padding; padded frames are zero rows) + caption ids [B, S]."""
    rng = np.random.default_rng(seed)
    feats, masks = [], []
    for i, (T, E) in enumerate(zip(Ts, shapes)):
        f = rng.standard_normal((B, T, E)).astype(np.float32)
        mk = np.zeros((B, T), bool)
        if valid is not None and valid[i] is not None:
            for b, n in enumerate(valid[i]):
                f[b, n:] = 0
                mk[b, n:] = True
        feats.append(f)
        masks.append(mk)
    ids = O.synthetic_batch(B, 2, 8, S, vocab, seed=seed + 7, ragged=True)[2]
    return feats, masks, ids
