"""float64 numpy restatement of what self-critical sequence training adds (include/vct_hip.h: vct_wce_loss, vct_group_sum;
vct_amd/rewards.py: CiderD).  Written from the definitions, with plain loops where the product code uses counters and
dictionaries of vectors; nothing here imports the product package."""
import math

import numpy as np


def wce_loss(logits, labels, seq_w, pad_id=0):
    """logits [N, V] (any float dtype, computed in float64); labels int [B, S] with N = B*S; seq_w [B] or None (all ones).
    Returns (loss, dlogits [N, V], tok_logp [N]):
        logp_n = x[y] - max - log(sum exp(x - max));   count = #(label != pad)
        loss = -(sum over valid n of w[n // S] * logp_n) / count;   tok_logp = logp_n on valid rows, 0 on pad rows
        dlogits[n] = (w[n // S] / count) * (softmax(x_n) - onehot(y_n)) on valid rows, 0 on pad rows."""
    x = np.asarray(logits, np.float64)
    lab = np.asarray(labels).reshape(-1)
    N, V = x.shape
    S = np.asarray(labels).shape[1]
    w = np.ones(N // S) if seq_w is None else np.asarray(seq_w, np.float64)
    valid = lab != pad_id
    count = int(valid.sum())
    loss = 0.0
    d = np.zeros((N, V))
    tok = np.zeros(N)
    for n in range(N):
        if not valid[n]:
            continue
        m = x[n].max()
        e = np.exp(x[n] - m)
        se = e.sum()
        logp = x[n, lab[n]] - m - math.log(se)
        tok[n] = logp
        loss -= w[n // S] * logp
        p = e / se
        p[lab[n]] -= 1.0
        d[n] = (w[n // S] / count) * p
    return (loss / count if count else float("nan")), d, tok


def group_sum(x, B, G, R):
    """x [B*G*R, d] -> [B*R, d]: out[g*R + r] = sum over n < G of x[(g*G + n)*R + r], in float64."""
    x = np.asarray(x, np.float64)
    return x.reshape(B, G, R, x.shape[1]).sum(1).reshape(B * R, x.shape[1])


# ---- CIDEr-D, directly from its definition --------------------------------------------------------------------------------------
def _cut(seq, end_id):
    out = []
    for t in seq:
        out.append(int(t))
        if int(t) == end_id:
            break
    return out


def _grams(seq, k):
    return [tuple(seq[i:i + k]) for i in range(len(seq) - k + 1)]


def cider_d(cand, vid, refs, n=4, sigma=6.0, end_id=102):
    """cand: token ids without the start token; refs {video: [id lists]}.  10 * mean over k = 1..n of mean over the video's references
    of  [sum_w min(c_w, r_w) * r_w / (|c| |r|)] * exp(-(len c - len r)^2 / (2 sigma^2)),  c_w = count_c(w) * idf(w),
    idf(w) = log(#videos) - log(max(1, #videos whose references contain w))."""
    cut_refs = {v: [_cut(r, end_id) for r in rs] for v, rs in refs.items()}
    c = _cut(cand, end_id)
    nvid = len(cut_refs)
    total = 0.0
    for k in range(1, n + 1):
        def idf(w):
            df = 0
            for v, rs in cut_refs.items():
                if any(w in _grams(r, k) for r in rs):
                    df += 1
            return math.log(nvid) - math.log(max(1, df))

        def vector(seq):
            g = _grams(seq, k)
            return {w: g.count(w) * idf(w) for w in set(g)}
        cv = vector(c)
        cn = math.sqrt(sum(v * v for v in cv.values()))
        acc = 0.0
        for r in cut_refs[vid]:
            rv = vector(r)
            rn = math.sqrt(sum(v * v for v in rv.values()))
            if cn == 0.0 or rn == 0.0:
                continue
            dot = 0.0
            for w in cv:
                if w in rv:
                    dot += min(cv[w], rv[w]) * rv[w]
            acc += dot / (cn * rn) * math.exp(-(len(c) - len(r)) ** 2 / (2.0 * sigma ** 2))
        total += acc / len(cut_refs[vid])
    return 10.0 * total / n


# ---- the whole model, n >= 1 feature streams, on the numpy oracle's layers (no fan-out: the caller repeats the features) ----------
def _mm_frontend(O, p, feats, dt):
    """MultiModalEncoder's input rows (aggregation 'avg', temporal 'encoding', do_norm False, modal_different True): per stream
    u_i = unify_i(x_i), rows [mean over ALL T_i frames, u_i]; the frames of stream i add pe[linspace(0, T_0 - 1, T_i) as int32], the
    aggregation rows nothing; with several streams every row adds its modal embedding (aggregation row of stream i: row i + n,
    frames: row i)."""
    n, d = len(feats), p[O.ENC + "unify.0.weight"].shape[0]
    pe = p[O.ENC + "temp_emb.pe"].reshape(-1, d).astype(dt)
    T0 = feats[0].shape[1]
    rows, labels = [], []
    for i, f in enumerate(feats):
        t = f.shape[1]
        u = O.linear(f.astype(dt), p[f"{O.ENC}unify.{i}.weight"].astype(dt), p[f"{O.ENC}unify.{i}.bias"].astype(dt))
        rows += [u.mean(1, keepdims=True), u + pe[np.linspace(0, T0 - 1, t).astype(np.int32)][None]]
        labels += [i + n] + [i] * t
    z = np.concatenate(rows, 1)
    if n > 1:
        z = z + p[O.ENC + "modal_emb.modal_emb.weight"].astype(dt)[np.array(labels)][None]
    return z, labels


def scst_loss_and_grads(O, p, cfg, feats, masks, ids, seq_w, dt=np.float64):
    """Weighted loss (wce_loss above) and every parameter gradient of the caption model on `ids` [M, L] with one weight per row;
    feats / masks: one array per stream, M rows each.  Encoder and decoder layers are vct_oracle's forward / backward."""
    n = len(feats)
    z, labels = _mm_frontend(O, p, feats, dt)
    M = z.shape[0]
    kpm = np.concatenate([np.concatenate([np.zeros((M, 1), bool), mk.astype(bool)], 1) for mk in masks], 1)
    add_mask = O._bool_to_add(kpm, dt)[:, None, None, :]
    x, caches = z, []
    for l in range(cfg["enc_layers"]):
        x, c = O.encoder_layer_fwd(p, f"{O.ENC}transformer_encoder.layers.{l}.", x, add_mask, cfg["enc_nhead"], cfg["activation"])
        caches.append(c)
    mem, c_norm = O.layer_norm(x, p[O.ENC + "transformer_encoder.norm.weight"].astype(dt), p[O.ENC + "transformer_encoder.norm.bias"].astype(dt))
    logits, _, c_dec = O.cap_decoder_forward(p, cfg, mem, ids, None, dt, return_cache=True)
    V = logits.shape[-1]
    loss, dlogits, tok = wce_loss(logits.reshape(-1, V), ids[:, 1:], seq_w, cfg.get("pad_id", 0))
    grads = {}
    dmem = O.cap_decoder_backward(c_dec[:4] + (dlogits.reshape(logits.shape).astype(dt),), p, cfg, grads, dt)
    dx, grads[O.ENC + "transformer_encoder.norm.weight"], grads[O.ENC + "transformer_encoder.norm.bias"] = \
        O.layer_norm_bwd(dmem, c_norm, p[O.ENC + "transformer_encoder.norm.weight"].astype(dt))
    for l in reversed(range(cfg["enc_layers"])):
        dx = O.encoder_layer_bwd(dx, caches[l], p, f"{O.ENC}transformer_encoder.layers.{l}.", cfg["enc_nhead"], cfg["activation"], grads)
    at = 0
    dmod = np.zeros((2 * n, dx.shape[-1]), dt)
    for s, lab in enumerate(labels):
        dmod[lab] += dx[:, s].sum(0)
    for i, f in enumerate(feats):
        t = f.shape[1]
        du = dx[:, at + 1:at + 1 + t] + dx[:, at:at + 1] / dt(t)
        _, grads[f"{O.ENC}unify.{i}.weight"], grads[f"{O.ENC}unify.{i}.bias"] = O.linear_bwd(du, f.astype(dt), p[f"{O.ENC}unify.{i}.weight"].astype(dt))
        at += t + 1
    if n > 1:
        grads[O.ENC + "modal_emb.modal_emb.weight"] = dmod
    return loss, grads, mem, tok.reshape(ids.shape[0], -1)
