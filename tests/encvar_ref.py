"""Shared by the encoder-variant tests and tools/make_golden_encoder_variants.py: the config block and the deterministic parameters
of a model whose `mme` block uses the learned temporal embedding, the max aggregation and / or the input norm (the fixtures record
only the seed)."""
import itertools

import numpy as np

import vct_oracle as O
from mm_ref import mm_config, mm_params

COMBOS = list(itertools.product(("avg", "max"), ("encoding", "embedding"), (False, True)))     # (aggregation, temporal, do_norm)


def encvar_config(shapes, aggregation="avg", temporal="encoding", do_norm=False, d=64, H=4, ff=128, Le=2, Ld=2, dropout=0.0):
    mc = mm_config(d, shapes, H, ff, Le, Ld, dropout=dropout)
    mc["video_encoder"]["mme"].update(aggregation=aggregation, temporal=temporal, do_norm=bool(do_norm))
    return mc


def combo_key(n, aggregation, temporal, do_norm):
    return f"{n}/{aggregation}/{temporal}/{int(bool(do_norm))}"


def encvar_params(mc, vocab, seed):
    """mm_params plus, as the options ask: temp_emb.embedding.weight [512, d] drawn N(0, 1) (nn.Embedding's init) INSTEAD of the
    `pe` buffer, and norm.weight = 1 + 0.05 N, norm.bias = 0.05 N (an affine part that is not the identity).  Both are drawn
    whatever the options are, so the parameters two variants share are equal."""
    p = mm_params(mc, vocab, seed)
    mme, d = mc["video_encoder"]["mme"], mc["embed_dim"]
    rng = np.random.default_rng(seed + 2000)
    emb = rng.standard_normal((512, d)).astype(np.float32)
    nw = (1.0 + 0.05 * rng.standard_normal(d)).astype(np.float32)
    nb = (0.05 * rng.standard_normal(d)).astype(np.float32)
    if mme.get("temporal", "encoding") == "embedding":
        del p[O.ENC + "temp_emb.pe"]
        p[O.ENC + "temp_emb.embedding.weight"] = emb
    if mme.get("do_norm", False):
        p[O.ENC + "norm.weight"], p[O.ENC + "norm.bias"] = nw, nb
    return p


def temporal_index(Ts):
    """TemporalEmbedding's row indices (model/MMEncoder.py:150-158 of the reference): 0 on aggregation rows, linspace(1, T_0, T_i)."""
    return np.concatenate([np.concatenate([np.zeros(1), np.linspace(1, Ts[0], t).astype(np.int32)]) for t in Ts]).astype(np.int64)
