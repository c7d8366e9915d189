"""Cost of the CLIP text tower (vct_amd.text.ClipTextTower) at the ViT-B/32 text shape -- 12 layers x width 512, 8 heads, ff 2048,
projection 512, vocabulary 49 408, random weights, bf16 -- with caption lengths drawn from 6 .. 25 tokens (start and EOT included).

    python tools/bench_text_tower.py [--captions 59800] [--chunk 1024] [--out profiles/text_tower_bench.jsonl]

Two workloads, each as the median of 9 timings between stream events after warm-up calls of every shape in the window:
  batch64   one training step's captions: encode_ids of 64 host id rows (the host trim and the id copy included)
  split     a whole split through encode_all (MSR-VTT: 59 800 captions), each chunk trimmed to its own L
and next to them, alternating with ours inside the same rounds, the same tower in torch on the same GPU: transformers'
CLIPTextModelWithProjection in bf16 where it imports, otherwise a torch.nn restatement on F.scaled_dot_product_attention.  The torch
side gets the same trimmed ids (ours is not credited with the trim).  One more line: the `match` training step of
tools/bench_matching.py at the same batch, so that the tower's share of a step can be stated.  Outputs of both sides are compared
(relative Frobenius) on the batch-64 ids, so a fast wrong answer cannot pass as a time."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPE = dict(W=512, H=8, ff=2048, layers=12, P=512, vocab=49408)


def make_ids(n, seed):
    """int64 [n, 77]: start token, words, EOT (the largest id) -- 6 .. 25 tokens in all."""
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(6, 26, (n,), generator=g)
    ids = torch.randint(1, SHAPE["vocab"] - 2, (n, 77), generator=g)
    col = torch.arange(77)[None]
    ids = torch.where(col < (lens[:, None] - 1), ids, torch.zeros_like(ids))
    ids[:, 0] = SHAPE["vocab"] - 2
    ids[torch.arange(n), lens - 1] = SHAPE["vocab"] - 1
    return ids


class TorchTower(torch.nn.Module):
    """The same tower on stock torch kernels, everything in bf16 (used where transformers does not import)."""

    def __init__(self, sd, H):
        super().__init__()
        import text_tower_ref as R
        w = R.weights(sd)
        bf = lambda t: torch.nn.Parameter(t.to(torch.bfloat16).cuda(), requires_grad=False)      # noqa: E731
        self.H = H
        self.tok, self.pos, self.lnf_g, self.lnf_b, self.proj = bf(w["tok"]), bf(w["pos"]), bf(w["lnf_g"]), bf(w["lnf_b"]), bf(w["proj"])
        self.lw = [{k: bf(v) for k, v in lw.items()} for lw in w["layers"]]

    @torch.no_grad()
    def forward(self, ids):
        B, L = ids.shape
        W = self.tok.shape[1]
        x = self.tok[ids] + self.pos[:L]
        for lw in self.lw:
            h = F.layer_norm(x, (W,), lw["ln1_g"], lw["ln1_b"], 1e-5)
            q, k, v = (t.reshape(B, L, self.H, -1).transpose(1, 2) for t in F.linear(h, lw["w_qkv"], lw["b_qkv"]).chunk(3, -1))
            o = F.scaled_dot_product_attention(q, k, v, is_causal=True).transpose(1, 2).reshape(B, L, W)
            x = x + F.linear(o, lw["w_o"], lw["b_o"])
            h = F.layer_norm(x, (W,), lw["ln2_g"], lw["ln2_b"], 1e-5)
            f = F.linear(h, lw["w_fc"], lw["b_fc"])
            x = x + F.linear(f * torch.sigmoid(1.702 * f), lw["w_proj"], lw["b_proj"])
        e = ids.argmax(-1)
        rows = F.layer_norm(x[torch.arange(B, device=ids.device), e], (W,), self.lnf_g, self.lnf_b, 1e-5)
        return (rows @ self.proj).float()


def torch_side(sd):
    """(name, callable ids_dev [B, L] -> fp32 [B, P])."""
    try:
        import text_tower_ref as R
        from transformers import CLIPTextConfig, CLIPTextModelWithProjection
        cfg = CLIPTextConfig(vocab_size=SHAPE["vocab"], hidden_size=SHAPE["W"], intermediate_size=SHAPE["ff"],
                             num_hidden_layers=SHAPE["layers"], num_attention_heads=SHAPE["H"], max_position_embeddings=77,
                             projection_dim=SHAPE["P"], hidden_act="quick_gelu", eos_token_id=2, bos_token_id=0, pad_token_id=1)
        m = CLIPTextModelWithProjection(cfg)
        m.load_state_dict(R.openai_to_transformers(sd), strict=False)
        m = m.to(torch.bfloat16).cuda().eval()

        @torch.no_grad()
        def run(ids):
            return m(input_ids=ids).text_embeds.float()
        return "transformers.CLIPTextModelWithProjection bf16", run
    except ImportError:
        t = TorchTower(sd, SHAPE["H"])
        return "torch.nn restatement (scaled_dot_product_attention) bf16", t


def median9(fns, warm=3):
    """The callables timed in turn inside each of 9 rounds (neighbours in time), each between stream events -> [(median, all)]."""
    for _ in range(warm):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(9):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts[k].append(e0.elapsed_time(e1))
    return [(sorted(t)[4], t) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--captions", type=int, default=59800)
    ap.add_argument("--chunk", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--no-match-step", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_text_tower.py measures on the GPU; there is none here")
    import text_tower_ref as R
    from vct_amd import text as T
    sd = R.random_state_dict(SHAPE["W"], SHAPE["H"], SHAPE["ff"], SHAPE["layers"], SHAPE["P"], SHAPE["vocab"], seed=1, std=0.03)
    tower = T.ClipTextTower.from_state_dict(sd, "cuda", torch.bfloat16)
    tname, ttower = torch_side(sd)
    ids64, ids_all = make_ids(args.batch, 2), make_ids(args.captions, 3)
    L64 = T.trim_length(ids64)
    ids64_dev = ids64[:, :L64].cuda()
    chunks = [ids_all[i:i + args.chunk] for i in range(0, args.captions, args.chunk)]
    chunks_dev = [c[:, :T.trim_length(c)].cuda() for c in chunks]
    out_all = torch.empty(args.captions, SHAPE["P"], device="cuda")

    ours64 = lambda: tower.encode_ids(ids64)                          # noqa: E731
    torch64 = lambda: ttower(ids64_dev)                               # noqa: E731
    ours_all = lambda: tower.encode_all(ids_all, chunk=args.chunk, out=out_all)      # noqa: E731

    def torch_all():
        for i, c in enumerate(chunks_dev):
            out_all[i * args.chunk:i * args.chunk + c.shape[0]] = ttower(c)
    a, b = ours64(), torch64()
    exact = R.tower(sd, ids64[:8], SHAPE["H"], L=L64).cuda()
    rel = lambda x, y: float((x.double() - y.double()).norm() / y.double().norm())      # noqa: E731
    recs = []
    res = {}
    for name, f_ours, f_torch, n in (("batch64", ours64, torch64, args.batch), ("split", ours_all, torch_all, args.captions)):
        warm = 3 if name == "batch64" else 1
        (mo, to), (mt, tt) = median9((f_ours, f_torch), warm)
        res[name] = (mo, mt)
        recs.append({"record": name, "captions": n, "chunk": args.chunk if name == "split" else None, "shape": SHAPE, "compute_dtype": "bf16",
                     "lengths": "6..25 tokens", "ours_ms_median9": round(mo, 4), "ours_ms_all": [round(t, 4) for t in to],
                     "torch_ms_median9": round(mt, 4), "torch_ms_all": [round(t, 4) for t in tt], "torch_side": tname,
                     "ours_over_torch": round(mo / mt, 4), "launches_per_call_ours": (7 * SHAPE["layers"] + 3) * (1 if name == "batch64" else len(chunks)),
                     "captions_per_s_ours": round(n / mo * 1e3, 1), "captions_per_s_torch": round(n / mt * 1e3, 1)})
    tower.check()
    recs.append({"record": "agreement_batch64", "L": L64, "rel_frobenius_ours_vs_torch": round(rel(a, b), 6),
                 "rel_frobenius_ours_vs_fp64_first8": round(rel(a[:8], exact), 6), "rel_frobenius_torch_vs_fp64_first8": round(rel(b[:8], exact), 6)})
    if not args.no_match_step:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import bench_matching as BM
        c = BM.Case("match", args.batch)
        for _ in range(3):
            c.run(30, 8)
        ms = sorted(c.times)[1]
        recs.append({"record": "match_step", "batch": args.batch, "ms_per_step_rounds": [round(t, 4) for t in c.times], "ms_per_step_median": round(ms, 4),
                     "tower_batch64_ms": round(res["batch64"][0], 4), "tower_over_match_step": round(res["batch64"][0] / ms, 4),
                     "note": "tools/bench_matching.py's match case (cfg-B model, eager executor) at this batch; the tower runs once per step in front of it"})
    out = args.out or os.path.join(ROOT, "profiles", "text_tower_bench.jsonl")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        for r in recs:
            f.write(json.dumps(r) + "\n")
            print(json.dumps(r))


if __name__ == "__main__":
    main()
