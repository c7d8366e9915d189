"""Generate tests/golden/mm_*.npz (multi-modal encoder input) from the REAL reference on CPU torch.

    python tools/make_golden_multimodal.py        # needs the reference checkout ($VCT_REFERENCE) and torch CPU

Modelled on oracle/make_golden.py and reusing its helpers unchanged (reference import, tokenizer / text-encoder stubs,
config builder).  Runs only where the reference checkout exists; no test runs it and no test reads the reference.
Fixtures hold inputs and outputs only.  Cases (model/MMEncoder.py:12-48, 83-104, 244-276 with n >= 2 modalities):
  A   tiny model, modal_shape [48, 24], T = (5, 3), padding in both modalities: everything (mm_train.npz, mm_train_adam.npz)
  A'  three modalities [48, 24, 16], modal_different false: loss, memory, unify.* / modal_emb gradients (mm_train3.npz)
  B   greedy ids of A's weights at B = 1 and 3, unpadded batches (mask None and all-False) (mm_decode.npz)
  C   d 512, 2 + 2 layers, V 30522, B 8, modal_shape [512, 128], T = (12, 8): slices only (mm_cfgC_slices.npz)
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
from mm_ref import mm_batch as batch, mm_config, mm_params  # noqa: E402

t2n = G.t2n


def run_train(mc, vocab, p, feats, masks, ids):
    m = G.build_ref(mc, vocab)
    G.load_np_state(m, p)
    m.train()
    rec = {}
    enc = m.video_encoder
    hooks = [enc.transformer_encoder.register_forward_pre_hook(lambda mod, a: rec.__setitem__("mm_src", t2n(a[0]))),
             enc.register_forward_hook(lambda mod, a, o: rec.update(memory=t2n(o[0]), gmask=t2n(o[1]), agg=t2n(o[2]))),
             m.cap_decoder.generator.register_forward_hook(lambda mod, a, o: rec.__setitem__("logits", t2n(o)))]
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


def greedy_ids(m, feats, masks, max_len=12):
    """The reference's greedy loop (MMT4Caption.py:146-172) replayed step by step to keep the whole id matrix."""
    with torch.no_grad():
        mem = m.video_encoder([torch.from_numpy(f) for f in feats], masks)[0]
        B = feats[0].shape[0]
        ys = torch.full((B, 1), 101, dtype=torch.long)
        flags = [0] * B
        for _ in range(max_len - 1):
            prob = m.cap_decoder.decode_word(mem, ys, None)
            nxt = torch.max(prob, dim=1)[1]
            ys = torch.cat([ys, nxt[:, None]], 1)
            for k, fl in enumerate((nxt == 102).tolist()):
                if fl:
                    flags[k] = 1
            if sum(flags) >= B:
                break
    return t2n(ys), t2n(mem)


def main():
    torch.set_num_threads(8)
    out = G.OUT
    summary = {}

    # ---------------- A. tiny, two modalities, padding in both ----------------
    V = 131
    mc = mm_config(64, [48, 24], 4, 128, 2, 2)
    p = mm_params(mc, V, 31)
    feats, masks, ids = batch(3, (5, 3), (48, 24), 7, V, seed=41, valid=[[5, 3, 4], [2, 3, 1]])
    loss, rec, grads, after, m = run_train(mc, V, p, feats, masks, ids)
    keys = {k: list(v.shape) for k, v in m.state_dict().items()}
    np.savez_compressed(
        os.path.join(out, "mm_train.npz"), model_config=json.dumps(mc), vocab=V, param_seed=31, state_keys=json.dumps(keys),
        feats0=feats[0], feats1=feats[1], mask0=masks[0], mask1=masks[1], ids=ids, loss=np.float64(loss),
        **{"act/" + k: v for k, v in rec.items()},
        **{"grad/" + k: v for k, v in grads.items()})
    # the parameters after one Adam step (lr 1e-4) in a file of their own: each fixture stays under 1 MB
    np.savez_compressed(os.path.join(out, "mm_train_adam.npz"), **{"adam1/" + k: v for k, v in after.items()})
    summary["mm_train.loss"] = loss

    # ---------------- A'. three modalities, modal_different false ----------------
    mc3 = mm_config(64, [48, 24, 16], 4, 128, 2, 2, modal_different=False)
    p3 = mm_params(mc3, V, 32)
    f3, k3, i3 = batch(3, (5, 3, 2), (48, 24, 16), 7, V, seed=42, valid=[[5, 4, 3], [3, 1, 2], None])
    loss3, rec3, grads3, _, m3 = run_train(mc3, V, p3, f3, k3, i3)
    np.savez_compressed(
        os.path.join(out, "mm_train3.npz"), model_config=json.dumps(mc3), vocab=V, param_seed=32,
        state_keys=json.dumps({k: list(v.shape) for k, v in m3.state_dict().items()}),
        **{f"feats{i}": f for i, f in enumerate(f3)}, **{f"mask{i}": k for i, k in enumerate(k3)}, ids=i3,
        loss=np.float64(loss3), memory=rec3["memory"],
        **{"grad/" + k: v for k, v in grads3.items() if ".unify." in k or ".modal_emb." in k})
    summary["mm_train3.loss"] = loss3

    # ---------------- B. greedy ids on A's weights, unpadded ----------------
    m.load_state_dict({k: torch.from_numpy(v) for k, v in p.items()}, strict=False)
    m.eval()
    dec = {}
    for tag, B in (("b1", 1), ("b3", 3)):
        fb, _, _ = batch(B, (5, 3), (48, 24), 4, V, seed=50 + B)
        ys_none, mem = greedy_ids(m, fb, None)
        ys_false, _ = greedy_ids(m, fb, [torch.zeros(B, 5, dtype=torch.bool), torch.zeros(B, 3, dtype=torch.bool)])
        assert np.array_equal(ys_none, ys_false)
        dec[f"{tag}/feats0"], dec[f"{tag}/feats1"], dec[f"{tag}/ys"], dec[f"{tag}/memory_eval"] = fb[0], fb[1], ys_none, mem
    np.savez_compressed(os.path.join(out, "mm_decode.npz"), param_seed=31, **dec)

    # ---------------- C. full width, two modalities, S = 22: slices only ----------------
    V2 = 30522
    mcC = mm_config(512, [512, 128], 8, 2048, 2, 2)
    pC = mm_params(mcC, V2, 33)
    fC, kC, iC = batch(8, (12, 8), (512, 128), 20, V2, seed=43, valid=[[12, 10, 12, 9, 12, 12, 11, 12], [8, 8, 6, 8, 7, 8, 8, 5]])
    lossC, recC, gradsC, afterC, _ = run_train(mcC, V2, pC, fC, kC, iC)
    names = sorted(gradsC)
    np.savez_compressed(
        os.path.join(out, "mm_cfgC_slices.npz"), model_config=json.dumps(mcC), vocab=V2, param_seed=33, batch_seed=43,
        loss=np.float64(lossC),
        memory_head=recC["memory"][:, :, :64], mm_src_head=recC["mm_src"][:, :, :64],
        logits_head=recC["logits"][:, :, :96], logits_argmax=recC["logits"].argmax(-1),
        grad_names=json.dumps(names),
        grad_norms=np.array([np.linalg.norm(gradsC[k].astype(np.float64)) for k in names]),
        grad_heads=np.stack([np.resize(gradsC[k].reshape(-1)[:32], 32) for k in names]),
        modal_emb_grad=gradsC["video_encoder.modal_emb.modal_emb.weight"],
        unify1_grad_head=gradsC["video_encoder.unify.1.weight"][:64])
    summary["mm_cfgC.loss"] = lossC
    print(json.dumps(summary, indent=1))
    for fn in sorted(os.listdir(out)):
        if fn.startswith("mm_"):
            print(fn, os.path.getsize(os.path.join(out, fn)))


if __name__ == "__main__":
    main()
