"""Generate tests/golden/hmm_*.npz / hmm_state_keys.json (video_encoder.type "hmme": the hierarchical multi-modal encoder) from the REAL
reference on CPU torch.

    python tools/make_golden_hmm_encoder.py     # needs the reference checkout ($VCT_REFERENCE) and torch CPU

Modelled on tools/make_golden_encoder_variants.py (its greedy loop and its max-aggregation guard are imported from there);
oracle/make_golden.py is imported unchanged for the reference import and the tokenizer / text-encoder stubs.  Runs only where the
reference checkout exists; no test runs it and no test reads the reference.  Fixtures hold inputs and outputs only; parameters are
recorded as a seed (tests/hmm_ref.py: different values per layer).  All cases: d 64, 4 heads, ff 128, 2 decoder layers, V 131, B 3,
padding as in mm_train.npz, dropout 0 (model/MMEncoder.py:313-402 of the reference):
  A   two streams [48, 24], T (5, 3), layer [2, 1]: the second stream restarts at layer 1
  B   two streams, layer [1, 3], 'embedding' + 'max' + do_norm: two mixed layers (the stack input's gradient sums three
      contributions on stream 0); plus the parameters after one Adam step (lr 1e-4) and greedy ids at B 1 and 3
  C   three streams [48, 24, 16], T (4, 1, 2), layer [3, 1, 2]
  D   one stream [48], T 5, layer [2]: no mixed layer, and no stack-final norm
each with loss, the input of every layer (forward pre-hooks on trans_enc_layers[i]; layer 0's is mm_src), memory, mask, agg_feats
([B]: the reference sums the concatenated first rows over dim 1) and every gradient; and the state_dict keys of layer [2, 1], [1, 3]
and [2] with and without the options (hmm_state_keys.json: the keys outside video_encoder once, the encoder's per entry).
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402  (puts the reference on sys.path)
from hmm_ref import hmm_config, hmm_params  # noqa: E402
from make_golden_encoder_variants import EMB, greedy_ids, max_gap, split_emb  # noqa: E402
from mm_ref import mm_batch  # noqa: E402

t2n = G.t2n
V, PARAM_SEED = 131, 37
OPTS = dict(aggregation="max", temporal="embedding", do_norm=True)


def run_train(mc, p, feats, masks, ids):
    m = G.build_ref(mc, V)
    G.load_np_state(m, p)
    m.train()
    rec = {"unify": {}}
    enc = m.video_encoder
    hooks = [enc.register_forward_hook(lambda mod, a, o: rec.update(memory=t2n(o[0]), gmask=t2n(o[1]), agg=t2n(o[2])))]
    for i, layer in enumerate(enc.trans_enc_layers):
        hooks.append(layer.register_forward_pre_hook(lambda mod, a, i=i: rec.__setitem__(f"layer_in{i}", t2n(a[0]))))
    for i, lin in enumerate(enc.unify):
        hooks.append(lin.register_forward_hook(lambda mod, a, o, i=i: rec["unify"].__setitem__(i, t2n(o))))
    opt = torch.optim.Adam(filter(lambda q: q.requires_grad, m.parameters()), lr=1e-4, betas=(0.9, 0.999))
    loss = m([torch.from_numpy(f) for f in feats], [torch.from_numpy(k) for k in masks], ids.tolist())
    opt.zero_grad()
    loss.backward()
    grads = {k: t2n(q.grad) for k, q in m.named_parameters() if q.grad is not None}
    opt.step()
    after = {k: t2n(q) for k, q in m.named_parameters() if q.requires_grad}
    for h in hooks:
        h.remove()
    return float(loss), rec, grads, after, m


def case(name, shapes, Ts, layers, valid, batch_seed, need_gap, **opts):
    mc = hmm_config(shapes, layers, **opts)
    p = hmm_params(mc, V, PARAM_SEED)
    while True:
        feats, masks, ids = mm_batch(3, Ts, shapes, 7, V, seed=batch_seed, valid=valid)
        loss, rec, grads, after, m = run_train(mc, p, feats, masks, ids)
        gap = max_gap(rec["unify"])
        if not need_gap or gap > 1e-3:
            break
        batch_seed += 1
    assert rec["agg"].shape == (3,) and len([k for k in rec if k.startswith("layer_in")]) == max(layers)
    enc_named = [k for k, _ in m.named_parameters() if k.startswith("video_encoder.")]
    assert all(k in grads and np.abs(grads[k]).max() > 0 for k in enc_named), "every encoder parameter gets a non-zero gradient"
    keys = {k: list(v.shape) for k, v in m.state_dict().items()}
    g, _ = split_emb(grads, Ts, "grad")
    extra = {}
    if EMB in grads:
        from encvar_ref import temporal_index
        rows = int(temporal_index(Ts).max()) + 1
        assert not grads[EMB][rows:].any() and np.array_equal(after[EMB][rows:], p[EMB][rows:])
        extra["emb_rows_read"] = np.array(sorted(set(temporal_index(Ts).tolist())))
    np.savez_compressed(
        os.path.join(G.OUT, f"hmm_{name}.npz"), model_config=json.dumps(mc), vocab=V, param_seed=PARAM_SEED, batch_seed=batch_seed,
        max_gap_rms=np.float64(gap), state_keys=json.dumps(keys), ids=ids, loss=np.float64(loss),
        **{f"feats{i}": f for i, f in enumerate(feats)}, **{f"mask{i}": k for i, k in enumerate(masks)},
        **{"act/" + k: v for k, v in rec.items() if k != "unify"}, **g, **extra)
    return mc, p, after, m, loss, gap, batch_seed


def main():
    torch.set_num_threads(8)
    summary = {}
    two = dict(shapes=[48, 24], Ts=(5, 3), valid=[[5, 3, 4], [2, 3, 1]], batch_seed=41)
    for name, kw in (("A", dict(two, layers=[2, 1], need_gap=False)),
                     ("C", dict(shapes=[48, 24, 16], Ts=(4, 1, 2), layers=[3, 1, 2], valid=[[4, 2, 3], [1, 1, 1], [2, 1, 2]], batch_seed=41,
                                need_gap=False)),
                     ("D", dict(shapes=[48], Ts=(5,), layers=[2], valid=[[5, 3, 4]], batch_seed=41, need_gap=False)),
                     ("B", dict(two, layers=[1, 3], need_gap=True, **OPTS))):
        mc, p, after, m, loss, gap, seed = case(name, **kw)
        summary[name] = dict(loss=loss, max_gap_rms=gap, batch_seed=seed)
    # B: the parameters after one Adam step, in a file of their own, and greedy ids on the ORIGINAL weights
    a, _ = split_emb(after, (5, 3), "adam1")
    np.savez_compressed(os.path.join(G.OUT, "hmm_B_adam.npz"), **a)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in p.items()}, strict=False)
    m.eval()
    dec = {}
    for tag, B in (("b1", 1), ("b3", 3)):
        fb, _, _ = mm_batch(B, (5, 3), (48, 24), 4, V, seed=50 + B)
        dec[f"{tag}/feats0"], dec[f"{tag}/feats1"], dec[f"{tag}/ys"] = fb[0], fb[1], greedy_ids(m, fb)
        with torch.no_grad():       # eval mode: masks=None and all-false masks agree
            a_ = m.video_encoder([torch.from_numpy(f) for f in fb], None)[0]
            b_ = m.video_encoder([torch.from_numpy(f) for f in fb], [torch.zeros(f.shape[:2], dtype=torch.bool) for f in fb])[0]
        assert float((a_ - b_).abs().max()) < 1e-5
    np.savez_compressed(os.path.join(G.OUT, "hmm_B_decode.npz"), param_seed=PARAM_SEED, **dec)
    # the state_dict surface
    keys = {"rest": None, "encoder": {}}
    for shapes, layers in (([48, 24], [2, 1]), ([48, 24], [1, 3]), ([48], [2])):
        for tag, opts in (("default", {}), ("options", OPTS)):
            r = G.build_ref(hmm_config(shapes, layers, **opts), V)
            got = {k: list(v.shape) for k, v in r.state_dict().items()}
            rest = {k: v for k, v in got.items() if not k.startswith("video_encoder.")}
            assert keys["rest"] in (None, rest)
            keys["rest"] = rest
            keys["encoder"][f"{layers}/{tag}"] = {k: v for k, v in got.items() if k.startswith("video_encoder.")}
    with open(os.path.join(G.OUT, "hmm_state_keys.json"), "w") as f:
        f.write("{\n \"rest\": " + json.dumps(keys["rest"], sort_keys=True) + ",\n \"encoder\": {\n"
                + ",\n".join(f"  {json.dumps(n)}: {json.dumps(k, sort_keys=True)}" for n, k in keys["encoder"].items()) + "\n }\n}\n")
    print(json.dumps(summary, indent=1))
    for fn in sorted(os.listdir(G.OUT)):
        if fn.startswith("hmm_"):
            print(fn, os.path.getsize(os.path.join(G.OUT, fn)))


if __name__ == "__main__":
    main()
