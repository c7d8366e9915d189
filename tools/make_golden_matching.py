"""Generate tests/golden/matching_*.npz / matching_state_keys.json (train.task "match" and "cross": the video-text matching head) from
the REAL reference on CPU torch.

    python tools/make_golden_matching.py     # needs the reference checkout ($VCT_REFERENCE) and torch CPU

Modelled on tools/make_golden_hmm_encoder.py; oracle/make_golden.py is imported unchanged for the reference import and the
tokenizer stub.  The reference's TextEncoder (a CLIP / BERT download) is replaced by a stub whose __call__ returns a recorded random
[B, dim] array and whose .dim is chosen per case.  Runs only where the reference checkout exists; no test runs it and no test
reads the reference.  Fixtures hold inputs and outputs only; parameters are recorded as a seed (tests/matching_ref.py).
All cases: d 64, 4 heads, ff 128, 1 encoder layer, 2 decoder layers, V 131, dropout 0, ragged padding as in mm_train.npz:
  P        match, CSL, fixed temperature 0.07; one stream [48], T 5, B 5; text dim 48 (v_proj present)
  L        match, CSL, learned temperature; two streams [48, 24], T (5, 3), B 3; text dim 64 (no v_proj); the temperature's gradient
  N        match, CSL, no temperature, B 3.  The reference never sets loss_fn.temperature for this block and raises AttributeError
           in forward; this tool sets `loss_fn.temperature = None` on the reference object -- the ONE line that makes the
           reference's own else branch (the plain similarity) reachable
  W_fixed  match, CSL_WDS, tau 0.5, B 5        W_learned  the same with a learned tau (initial 1.0)
  X        cross, loss_beta 0.3, CSL with a learned temperature, two streams, text dim 48, B 3
each with text_feats, agg (the encoder's agg_feat) and dagg (its gradient), vid (after v_proj), sim (the matrix the cross-entropies saw), the loss (X: also
cap_loss and match_loss), every parameter gradient, the names of the parameters that got none, and the parameters after one
torch.optim.Adam step (lr 1e-4) over filter(requires_grad) (X: in matching_X_adam.npz); and the matching.* state_dict keys of every temperature form.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
import make_golden as G  # noqa: E402  (puts the reference on sys.path)
from matching_ref import matching_block, matching_config, matching_params  # noqa: E402
from mm_ref import mm_batch  # noqa: E402

t2n = G.t2n
V, PARAM_SEED = 131, 53


def build_ref(mc, text_feats):
    """The reference model with the tokenizer stub and a text-encoder stub that returns `text_feats`."""
    G.RM.CapPreprocessor = G.make_prep(V)

    class StubText:
        def __init__(self, *_a, **_k):
            self.dim = mc["text_enc_dim"]

        def __call__(self, _captions):
            return torch.from_numpy(text_feats)
    G.RM.TextEncoder = StubText
    return G.RM.MMT4Caption(mc, device=G.CPU)


def case(name, task, shapes, Ts, valid, B, text_dim, matching, batch_seed, loss_beta=0.5, no_temperature=False):
    mc = matching_config(shapes, text_dim, matching, loss_beta=loss_beta)
    p = matching_params(mc, V, PARAM_SEED)
    feats, masks, ids = mm_batch(B, Ts, shapes, 7, V, seed=batch_seed, valid=valid)
    text = np.random.default_rng(batch_seed + 500).standard_normal((B, text_dim)).astype(np.float32)
    m = build_ref(mc, text)
    if no_temperature:
        m.matching.loss_fn.temperature = None
    m.mode(task)
    G.load_np_state(m, p)
    m.train()
    rec = {}
    def enc_hook(_mod, _a, o):
        o[2].retain_grad()                  # agg_feat = memory[:, 0]: its gradient is the head's d(loss)/d(agg) (X: times 1 - loss_beta)
        rec.update(memory=t2n(o[0]), agg=t2n(o[2]), agg_t=o[2])
    hooks = [m.video_encoder.register_forward_hook(enc_hook),
             m.matching.loss_fn.register_forward_pre_hook(lambda mod, a: rec.update(vid=t2n(a[1]))),
             m.matching.loss_fn.cross_entropy.register_forward_pre_hook(
                 lambda mod, a: None if "sim" in rec else rec.update(sim=t2n(a[0])))]      # (the first call: the text-major matrix)
    opt = torch.optim.Adam(filter(lambda q: q.requires_grad, m.parameters()), lr=1e-4, betas=(0.9, 0.999))
    out = m([torch.from_numpy(f) for f in feats], [torch.from_numpy(k) for k in masks], ids.tolist())
    loss = out[0] if task == "cross" else out
    opt.zero_grad()
    loss.backward()
    grads = {k: t2n(q.grad) for k, q in m.named_parameters() if q.grad is not None}
    none = [k for k, q in m.named_parameters() if q.grad is None]
    opt.step()
    after = {k: t2n(q) for k, q in m.named_parameters() if q.requires_grad}
    for h in hooks:
        h.remove()
    assert rec["agg"].shape == (B, 64) and rec["sim"].shape == (B, B)
    if task == "match":
        assert all(k.startswith("cap_decoder.") for k in none) and any(k.startswith("cap_decoder.") for k in none)
    else:
        assert not none
    losses = {"loss": np.float64(float(loss))}
    if task == "cross":
        losses.update(cap_loss=np.float64(float(out[1])), match_loss=np.float64(float(out[2])))
    np.savez_compressed(
        os.path.join(G.OUT, f"matching_{name}.npz"), model_config=json.dumps(mc), task=task, vocab=V, param_seed=PARAM_SEED,
        batch_seed=batch_seed, ids=ids, text_feats=text, agg=rec["agg"], vid=rec["vid"], sim=rec["sim"], dagg=t2n(rec["agg_t"].grad),
        no_grad=json.dumps(none),
        **losses, **{f"feats{i}": f for i, f in enumerate(feats)}, **{f"mask{i}": k for i, k in enumerate(masks)},
        **{"grad/" + k: v for k, v in grads.items()}, **({} if task == "cross" else {"adam1/" + k: v for k, v in after.items()}))
    if task == "cross":       # (every parameter is trainable: the stepped parameters go to a file of their own, like hmm_B_adam.npz)
        np.savez_compressed(os.path.join(G.OUT, f"matching_{name}_adam.npz"), **{"adam1/" + k: v for k, v in after.items()})
    return {k: float(v) for k, v in losses.items()}


def main():
    torch.set_num_threads(8)
    one5 = dict(shapes=[48], Ts=(5,), valid=[[5, 3, 4, 2, 5]], B=5, text_dim=48)
    one3 = dict(shapes=[48], Ts=(5,), valid=[[5, 3, 4]], B=3, text_dim=48)
    two3 = dict(shapes=[48, 24], Ts=(5, 3), valid=[[5, 3, 4], [2, 3, 1]], B=3)
    summary = {
        "P": case("P", "match", matching=matching_block("CSL", "fixed", 0.07), batch_seed=61, **one5),
        "L": case("L", "match", matching=matching_block("CSL", "learned"), batch_seed=62, text_dim=64, **two3),
        "N": case("N", "match", matching=matching_block("CSL", "none"), batch_seed=63, no_temperature=True, **one3),
        "W_fixed": case("W_fixed", "match", matching=matching_block("CSL_WDS", "fixed", 0.5), batch_seed=64, **one5),
        "W_learned": case("W_learned", "match", matching=matching_block("CSL_WDS", "learned"), batch_seed=65, **one5),
        "X": case("X", "cross", matching=matching_block("CSL", "learned"), batch_seed=66, text_dim=48, loss_beta=0.3, **two3),
    }
    # the state_dict surface of matching.* in every temperature form, with and without v_proj
    keys = {}
    for kind in ("CSL", "CSL_WDS"):
        for form in ("none", "fixed", "learned"):
            for dim in (48, 64):
                r = build_ref(matching_config([48], dim, matching_block(kind, form, 0.5)), None)
                keys[f"{kind}/{form}/text{dim}"] = {k: list(v.shape) for k, v in r.state_dict().items() if k.startswith("matching.")}
    with open(os.path.join(G.OUT, "matching_state_keys.json"), "w") as f:
        f.write("{\n" + ",\n".join(f" {json.dumps(n)}: {json.dumps(k, sort_keys=True)}" for n, k in keys.items()) + "\n}\n")
    print(json.dumps(summary, indent=1))
    for fn in sorted(os.listdir(G.OUT)):
        if fn.startswith("matching_"):
            print(fn, os.path.getsize(os.path.join(G.OUT, fn)))


if __name__ == "__main__":
    main()
