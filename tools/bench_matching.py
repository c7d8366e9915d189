"""Cost of the video-text matching task at cfg-B (d 512, 2 + 2 layers, V 30522, batch 256, bf16, 12 frames, captions of 20 tokens) on the
EAGER executor -- the only one the match / cross tasks run on.  The head: v_proj 512 -> 768 (text_enc_type "BERT"), CSL with a learned
temperature.

    python tools/bench_matching.py [--steps 30] [--warmup 8] [--rounds 3] [--out profiles/matching_bench.jsonl]

Training step time, same process and same build, in alternating rounds (a round runs every case once, so a ratio compares
neighbours in time):
  caption   the caption step, eager (the optimizer inside the weight-gradient GEMMs, as the eager caption step has it)
  cross     both tasks: the caption forward, the head, the non-overlapped backward, the gradient mix, the separate optimizer pass
  match     the match task: encoder + head only
Per case one JSON line: ms/step per round, the median, the ratio to `caption` and `caption`'s own spread over the rounds.  One more line:
the head's launches of one step (aggregation rows, v_proj, the loss chain, the two v_proj backward GEMMs, the aggregation rows'
backward) issued back to back on an otherwise idle GPU, bracketed by events -- NOT their time inside a step."""
import argparse
import copy
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

TASKS = ("caption", "cross", "match")


def model_for(task):
    from vct_amd.model import MMT4Caption
    mc = copy.deepcopy(bench.MODEL_CFG)
    mc["text_enc_type"] = "BERT"
    mc["matching"] = {"enable_tem": True, "matching_loss": "CSL"}
    torch.manual_seed(666)
    m = MMT4Caption(mc, device=torch.device("cuda"), compute_dtype=torch.bfloat16)
    m.mode(task)
    return m


class Case:
    def __init__(self, task, B):
        from vct_amd.trainer import CaptionTrainer, build_optimizer
        self.name = task
        self.model = model_for(task)
        self.model.train()
        opt, _ = build_optimizer(bench.TRAIN_CFG, self.model)
        self.trainer = CaptionTrainer(self.model, opt, None, use_graph=False, launch_list=False)
        feats, mask, ids = bench.synthetic(B, 0, "cuda")
        text = torch.randn(B, self.model.text_encoder.dim, generator=torch.Generator().manual_seed(1)).cuda()
        self.inputs = (feats, mask, ids) if task == "caption" else (feats, mask, ids, text)
        self.trainer.step(*self.inputs)
        self.times = []

    def run(self, steps, warmup):
        for _ in range(warmup):
            self.trainer.step(*self.inputs)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            self.trainer.step(*self.inputs)
        torch.cuda.synchronize()
        self.times.append((time.perf_counter() - t0) / steps * 1e3)


def head_alone(model, B, reps):
    """The head's launches of one match step on buffers of the step's shape, back to back: launches per step and microseconds."""
    from vct_amd import ops
    Te, d = bench.T_FRAMES + 1, 512
    mem = torch.randn(B * Te, d, device="cuda").to(torch.bfloat16)
    dmem = torch.empty_like(mem)
    text = torch.randn(B, model.text_encoder.dim, device="cuda")
    mt, g = model.matching, model._ps.g
    agg = torch.empty(B, d, device="cuda")
    dagg = torch.empty(B, d, device="cuda")

    def head():
        ops.match_agg_fwd(mem, agg, B, Te)
        st = mt.head_forward(text, agg, backward=True)
        mt.head_backward(st, dagg, g["matching.v_proj.weight"], g["matching.v_proj.bias"])
        ops.axpby(g["matching.loss_fn.temperature"], st["dtemp"], 1.0)
        ops.match_agg_bwd(dmem, dagg, B, Te, 0.0, empty=True)
    for _ in range(10):
        head()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        head()
    e1.record()
    torch.cuda.synchronize()
    # aggregation rows 1, v_proj 1, loss chain 4 (CSL, with backward), v_proj dX and dW 2, temperature gradient 1, aggregation rows' backward 1
    return {"record": "head_launches_alone", "batch": B, "text_dim": model.text_encoder.dim, "loss": "CSL", "launches": 10, "reps": reps,
            "us_per_head": round(e0.elapsed_time(e1) * 1e3 / reps, 2),
            "note": "back to back on an idle GPU, Python and launch gaps included; not the time inside a step"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--head-reps", type=int, default=200)
    ap.add_argument("--out", default=None, help="JSON lines (default profiles/matching_bench.jsonl)")
    args = ap.parse_args()
    cases = [Case(t, args.batch) for t in TASKS]
    for _ in range(args.rounds):
        for c in cases:
            c.run(args.steps, args.warmup)
    med = {c.name: sorted(c.times)[len(c.times) // 2] for c in cases}
    base = cases[0]
    out = args.out or os.path.join(ROOT, "profiles", "matching_bench.jsonl")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        for c in cases:
            rec = {"record": "train_step", "case": c.name, "batch": args.batch, "executor": "eager", "compute_dtype": "bf16",
                   "adam_in_dw_gemms": bool(c.trainer.fuse_adam), "steps": args.steps, "rounds": args.rounds,
                   "ms_per_step_rounds": [round(t, 4) for t in c.times], "ms_per_step_median": round(med[c.name], 4),
                   "over_caption": round(med[c.name] / med[base.name], 4),
                   "caption_spread": round((max(base.times) - min(base.times)) / med[base.name], 4)}
            f.write(json.dumps(rec) + "\n")
            print(json.dumps(rec))
        rec = head_alone(cases[2].model, args.batch, args.head_reps)
        f.write(json.dumps(rec) + "\n")
        print(json.dumps(rec))


if __name__ == "__main__":
    main()
