"""float64 numpy restatement of the video-text matching head (reference: model/Matching.py, model/loss.py), shared by the matching
tests and tools/make_golden_matching.py: v_proj, the L2 normalisation, both losses in all four temperature forms, and the gradients
with respect to vid, v_proj, the temperature and agg.  sim[i, j] = t^_i . v^_j: text rows, video columns."""
import json
import math

import numpy as np

TEMP_FORMS = ("none", "fixed", "learned")


def _lse(a, axis):
    m = a.max(axis=axis, keepdims=True)
    return (m + np.log(np.exp(a - m).sum(axis=axis, keepdims=True))).squeeze(axis)


def normalise(x):
    x = np.asarray(x, np.float64)
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def logits_of(text, vid, kind, temp):
    """(logits the two cross-entropies see, sim, softmax prior P or None).  kind 'CSL': temp None = plain sim, else sim * exp(temp);
    'CSL_WDS': sim * softmax(sim / temp, over the text index) * B."""
    S = normalise(text) @ normalise(vid).T
    B = S.shape[0]
    if kind == "CSL":
        return (S * math.exp(temp) if temp is not None else S), S, None
    Z = S / temp
    P = np.exp(Z - _lse(Z, 0)[None, :])
    return S * P * B, S, P


def loss_of(A):
    B = A.shape[0]
    d = np.diag(A)
    return float(((_lse(A, 1) - d).mean() + (_lse(A, 0) - d).mean()) / 2)


def head(text, vid, kind="CSL", temp=None, want_grad=True):
    """loss, logits and (want_grad) d(loss)/d(vid) [B, Dt] through the normalisation, d(loss)/d(temp) with the sum of the absolute
    values of its terms (None without a temperature)."""
    text, vid = np.asarray(text, np.float64), np.asarray(vid, np.float64)
    A, S, P = logits_of(text, vid, kind, temp)
    B = A.shape[0]
    out = {"loss": loss_of(A), "sim": A}
    if not want_grad:
        return out
    G = (np.exp(A - _lse(A, 1)[:, None]) + np.exp(A - _lse(A, 0)[None, :]) - 2 * np.eye(B)) / (2 * B)      # d(loss) / d(logits)
    if kind == "CSL":
        s = math.exp(temp) if temp is not None else 1.0
        dS = G * s
        terms = G * A if temp is not None else None              # d(logits) / d(temp) = logits
    else:
        H = G * B * S                                            # d(loss) / dP
        dZ = P * (H - (P * H).sum(0, keepdims=True))
        dS = G * B * P + dZ / temp
        terms = -dZ * S / (temp * temp)
    vn = np.linalg.norm(vid, axis=-1, keepdims=True)
    vh, th = vid / vn, normalise(text)
    dvh = dS.T @ th
    out["dvid"] = (dvh - vh * (vh * dvh).sum(-1, keepdims=True)) / vn
    out["dtemp"] = float(terms.sum()) if terms is not None else None
    out["dtemp_abs"] = float(np.abs(terms).sum()) if terms is not None else None
    return out


def head_with_proj(text, agg, W=None, b=None, kind="CSL", temp=None):
    """The whole Matching.forward: vid = agg @ W^T + b when v_proj exists.  Adds dagg, dW, db to head()'s results."""
    agg = np.asarray(agg, np.float64)
    vid = agg @ np.asarray(W, np.float64).T + np.asarray(b, np.float64) if W is not None else agg
    out = head(text, vid, kind, temp)
    out["vid"] = vid
    if W is not None:
        out["dagg"] = out["dvid"] @ np.asarray(W, np.float64)
        out["dW"] = out["dvid"].T @ agg
        out["db"] = out["dvid"].sum(0)
    else:
        out["dagg"] = out["dvid"]
    return out


def matching_block(kind="CSL", form="none", tau=None):
    """model_config['matching'] for a loss kind and a temperature form ('none' | 'fixed' | 'learned')."""
    blk = {"enable_tem": form == "learned", "matching_loss": kind}
    if form == "fixed":
        blk["temperature"] = float(tau)
    return blk


def matching_config(shapes, text_dim, matching, loss_beta=0.5, d=64, H=4, ff=128, Le=1, Ld=2):
    """cfg['model'] of the fixtures' cases; `text_enc_dim` is this project's key for a text encoder that is neither CLIP nor BERT."""
    return {"modal": [f"m{i}" for i in range(len(shapes))], "modal_shape": list(shapes), "tokenizer": "stub", "text_enc_type": "CLIP",
            "text_enc_dim": int(text_dim), "embed_dim": d, "dropout": 0.0, "loss_beta": loss_beta, "matching": matching,
            "activation": "gelu",
            "video_encoder": {"layer": Le, "nhead": H, "feedforward": ff,
                              "mme": {"temporal": "encoding", "modal_different": True, "do_norm": False, "aggregation": "avg"}},
            "caption_decoder": {"layer": Ld, "nhead": H, "feedforward": ff, "sce_loss_alpha": 0.5}, "pretrained_model": None}


def matching_params(mc, vocab, seed):
    """mm_ref.mm_params plus matching.v_proj.* (nn.Linear-like uniform) when the widths differ; the learned temperature keeps its
    initial 1.0 (it is not in this dict)."""
    from mm_ref import mm_params
    p = mm_params(mc, vocab, seed)
    d, dt = mc["embed_dim"], mc["text_enc_dim"]
    if d != dt:
        rng = np.random.default_rng(seed + 2000)
        bound = 1.0 / math.sqrt(d)
        p["matching.v_proj.weight"] = rng.uniform(-bound, bound, (dt, d)).astype(np.float32)
        p["matching.v_proj.bias"] = rng.uniform(-bound, bound, (dt,)).astype(np.float32)
    return p


def temp_of(z):
    """The temperature value a fixture's loss saw (None: the plain similarity)."""
    blk = json.loads(str(z["model_config"]))["matching"]
    if blk.get("temperature") is not None:
        return float(blk["temperature"])
    return 1.0 if blk["enable_tem"] else None
