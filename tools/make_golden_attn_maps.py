"""Generate tests/golden/attnmap_train.npz (cross-attention maps of the reference's Vis decoder) from the REAL reference on CPU torch.

    python tools/make_golden_attn_maps.py     # needs the reference checkout ($VCT_REFERENCE) and torch CPU

Modelled on tools/make_golden_encoder_variants.py; oracle/make_golden.py is imported unchanged for the reference import and the
tokenizer / text-encoder stubs.  Runs only where the reference checkout exists; no test runs it and no test reads the reference.
The fixture holds inputs and outputs only; parameters are recorded as a seed (vct_oracle.init_params).

Model: d 64, 4 heads, ff 128, 2 + 2 layers, V 131, one stream [48], B 3, T 5 (Te 6), S 7, `caption_decoder.layer_type: "vis"`
(model/CapDecoder.py:17-24, 83-154), dropout 0, train() mode.  Padding as in tiny_train.npz: a short caption (sample 1: four tokens)
and a padded video (sample 2: two padded frames).  Contents:
  feats, mask, ids           the batch
  loss, act/logits           what the forward returns
  attn0, attn1               cap_decoder.attn_weights (CapDecoder.py:53-54): fp32 [B, S-1, Te] per layer, head-averaged
  act/memory, act/ca_in0     the encoder memory and the input of layer 0's multihead_attn (norm1's output): with the seed's
                             in_proj they give that layer's q and K projections, so tests/attnmap_ref.py can be held to attn0
  state_keys                 the Vis model's state_dict keys / shapes (asserted equal to the plain decoder's here)
  greedy/ys                  the greedy id matrix on the same features (no mask, max_len 12) -- computed on a PLAIN-decoder
                             reference model with the same weights: the reference's decode_word indexes the Vis decoder's
                             (output, weights) tuple and fails on it, which is why predict_video.py patches plain layers instead
A decode step has no key-padding mask in self-attention while training has one, so a decode map row can be compared with attn*[b,
t-1] only up to the sample's first pad: the tool asserts every sample leaves at least 4 such rows, and that every row sums to 1
within 1e-6.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
import make_golden as G  # noqa: E402  (puts the reference on sys.path)
import vct_oracle as O  # noqa: E402

t2n = G.t2n
V, PARAM_SEED, BATCH_SEED = 131, 17, 9


def main():
    torch.set_num_threads(8)
    mc = G.model_cfg(d=64, d_in=48, H=4, ff=128, Le=2, Ld=2, alpha=0.5)
    plain = json.loads(json.dumps(mc))
    mc["caption_decoder"]["layer_type"] = "vis"
    p = O.init_params(O.cfg_from_model_config(mc, V), seed=PARAM_SEED)
    feats, mask, ids = O.synthetic_batch(3, 5, 48, 7, V, seed=BATCH_SEED, ragged=True)
    ids[1, 4:] = 0; ids[1, 3] = 102          # a short caption -> pad rows
    mask[2, 3:] = True; feats[2, 3:] = 0     # a padded video
    first_pad = [int(np.argmax(r == 0)) if (r == 0).any() else len(r) for r in ids[:, :-1]]
    assert min(first_pad) >= 4, first_pad    # comparable decode rows per sample

    m = G.build_ref(mc, V)
    G.load_np_state(m, p)
    m.train()
    rec = {}
    hooks = [m.video_encoder.register_forward_hook(lambda mod, a, o: rec.__setitem__("memory", t2n(o[0]))),
             m.cap_decoder.decoder.layers[0].multihead_attn.register_forward_pre_hook(lambda mod, a: rec.__setitem__("ca_in0", t2n(a[0]))),
             m.cap_decoder.generator.register_forward_hook(lambda mod, a, o: rec.__setitem__("logits", t2n(o)))]
    loss = m([torch.from_numpy(feats)], [torch.from_numpy(mask)], ids.tolist())
    for h in hooks:
        h.remove()
    attn = [t2n(a) for a in m.cap_decoder.attn_weights]
    assert len(attn) == 2 and all(a.shape == (3, 6, 6) and a.dtype == np.float32 for a in attn)
    dev = max(float(np.abs(a.astype(np.float64).sum(-1) - 1.0).max()) for a in attn)
    assert dev < 1e-6, dev
    keys = {k: list(v.shape) for k, v in m.state_dict().items()}

    mp = G.build_ref(plain, V)
    assert {k: list(v.shape) for k, v in mp.state_dict().items()} == keys
    G.load_np_state(mp, p)
    mp.eval()
    with torch.no_grad():
        mem = mp.video_encoder([torch.from_numpy(feats)], None)[0]
        ys = torch.full((3, 1), 101, dtype=torch.long)
        flags = [0] * 3
        for _ in range(11):
            nxt = torch.max(mp.cap_decoder.decode_word(mem, ys, None), dim=1)[1]
            ys = torch.cat([ys, nxt[:, None]], 1)
            for k, fl in enumerate((nxt == 102).tolist()):
                if fl:
                    flags[k] = 1
            if sum(flags) >= 3:
                break

    out = os.path.join(G.OUT, "attnmap_train.npz")
    np.savez_compressed(out, model_config=json.dumps(mc), vocab=V, param_seed=PARAM_SEED, batch_seed=BATCH_SEED,
                        state_keys=json.dumps(keys), feats=feats, mask=mask, ids=ids, loss=np.float64(float(loss)),
                        attn0=attn[0], attn1=attn[1], first_pad=np.array(first_pad),
                        **{"act/" + k: v for k, v in rec.items()}, **{"greedy/ys": t2n(ys)})
    print(json.dumps(dict(loss=float(loss), row_sum_dev=dev, first_pad=first_pad, greedy_len=int(ys.shape[1]))))
    print(out, os.path.getsize(out))


if __name__ == "__main__":
    main()
