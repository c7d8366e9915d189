"""Cost of the hierarchical multi-modal encoder (video_encoder.type "hmme") at cfg-B (d 512, 2 decoder layers, V 30522, batch 256, bf16,
captions of 20 tokens), two streams [512, 128] with T (12, 8) (S = 22 memory rows), hipGraph executor.

    python tools/bench_hmm_encoder.py [--steps 30] [--warmup 8] [--rounds 3] [--out profiles/hmm_encoder_bench.jsonl]

Training step time, same process and same build, measured in alternating rounds (a round runs every case once, so a ratio compares
neighbours in time):
  mme_2            `mme`, 2 layers: the encoder stack runs sample-stationary (one launch)
  mme_2_unfused    the same model with the ENCODER's stack forced layer by layer (its engine's fuse_layers switch; the decoder keeps its
                   own path): what leaving the sample-stationary stack costs, separated from the routing
  hmme_2_2         `hmme` [2, 2]: the unfused schedule without a final norm and without a mix launch
  hmme_2_1         `hmme` [2, 1]: one forward and two backward mix launches
Per case one JSON line: ms/step per round, the median, the ratio to mme_2 and mme_2's own spread over the rounds.  For hmme_2_1 one
more line: the bytes its three mix launches request (bf16 rows, fp32 accumulator) and the time of that trio issued back to back on
an otherwise idle GPU, bracketed by events around `--mix-reps` repetitions -- NOT their time inside the step, where they sit on the
side stream beside other kernels."""
import argparse
import copy
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench  # noqa: E402
from bench_multimodal import batch_for  # noqa: E402

SHAPES, TS = [512, 128], (12, 8)
CASES = {"mme_2": ("mme", 2, True), "mme_2_unfused": ("mme", 2, False), "hmme_2_2": ("hmme", [2, 2], True),
         "hmme_2_1": ("hmme", [2, 1], True)}


def model_for(enc_type, layer):
    from vct_amd.model import MMT4Caption
    mc = copy.deepcopy(bench.MODEL_CFG)
    mc["modal"], mc["modal_shape"] = [f"m{i}" for i in range(len(SHAPES))], list(SHAPES)
    mc["video_encoder"].update(type=enc_type, layer=layer)
    torch.manual_seed(666)
    m = MMT4Caption(mc, device=torch.device("cuda"), compute_dtype=torch.bfloat16)
    m.mode("caption")
    return m


class Case:
    def __init__(self, name, B):
        from vct_amd import engine
        from vct_amd.trainer import CaptionTrainer, build_optimizer
        enc_type, layer, fused = CASES[name]
        self.name = name
        self.model = model_for(enc_type, layer)
        self.model.train()
        if not fused:
            self.model.video_encoder._engine().fuse_layers = False
        o, _ = build_optimizer(bench.TRAIN_CFG, self.model)
        self.trainer = CaptionTrainer(self.model, o, None, use_graph=True, launch_list=False)
        self.inputs = self.trainer.adopt_inputs(*batch_for(SHAPES, TS, B))
        seen, orig = [], engine._StackBase._stack_ss

        def spy(eng, *a, **k):
            seen.append(type(eng).__name__)
            return orig(eng, *a, **k)
        engine._StackBase._stack_ss = spy
        try:
            self.trainer.step(*self.inputs)          # eager first step (allocates, then captures), records which stacks were fused
        finally:
            engine._StackBase._stack_ss = orig
        self.ss = sorted(set(seen))
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


def mix_alone(B, reps, d=512):
    """The three mix launches of one hmme [2, 1] step (forward at layer 1; backward INIT at layer 1, the closing form at layer 0) on
    buffers of the step's shape: bytes requested and microseconds per trio."""
    from vct_amd import ops
    from vct_amd.engine import HMMEncoderEngine
    S = sum(t + 1 for t in TS)
    take = torch.from_numpy(HMMEncoderEngine.take_table([2, 1], TS)).cuda()[1]
    rows = [torch.randn(B * S, d, device="cuda").to(torch.bfloat16) for _ in range(6)]
    acc = torch.empty(B * S, d, device="cuda")

    def trio():
        ops.hmm_mix_fwd(rows[0], rows[1], take, rows[2], B, S)
        ops.hmm_mix_bwd(rows[3], take, acc, B, S, dy=rows[4], init=True)
        ops.hmm_mix_bwd(rows[3], None, acc, B, S, dx0=rows[5])
    for _ in range(10):
        trio()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        trio()
    e1.record()
    torch.cuda.synchronize()
    n = B * S * d
    # fwd: one row read + one written (2 B each); bwd INIT: dx read, dy written, acc written in full (4 B); closing: dx + acc read, dx0 written
    nbytes = (2 * n + 2 * n) + (2 * n + 2 * n + 4 * n) + (2 * n + 4 * n + 2 * n)
    us = e0.elapsed_time(e1) * 1e3 / reps
    return {"record": "mix_launches_alone", "case": "hmme_2_1", "batch": B, "S": S, "d": d, "launches": 3, "reps": reps,
            "bytes_requested": nbytes, "us_per_trio": round(us, 2), "GBps": round(nbytes / (us * 1e-6) / 1e9, 1),
            "note": "back to back on an idle GPU, launch gaps included; not the time inside the step"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--mix-reps", type=int, default=200)
    ap.add_argument("--out", default=None, help="JSON lines (default profiles/hmm_encoder_bench.jsonl)")
    args = ap.parse_args()
    cases = [Case(n, args.batch) for n in CASES]
    for _ in range(args.rounds):
        for c in cases:
            c.run(args.steps, args.warmup)
    med = {c.name: sorted(c.times)[len(c.times) // 2] for c in cases}
    base = cases[0]
    out = args.out or os.path.join(ROOT, "profiles", "hmm_encoder_bench.jsonl")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        for c in cases:
            enc_type, layer, _ = CASES[c.name]
            rec = {"record": "train_step", "case": c.name, "encoder": enc_type, "layer": layer, "batch": args.batch, "modal_shape": SHAPES,
                   "T": list(TS), "executor": "graph" if c.trainer.use_graph else "eager (capture failed)", "steps": args.steps,
                   "rounds": args.rounds, "ms_per_step_rounds": [round(t, 4) for t in c.times], "ms_per_step_median": round(med[c.name], 4),
                   "over_mme_2": round(med[c.name] / med[base.name], 4),
                   "mme_2_spread": round((max(base.times) - min(base.times)) / med[base.name], 4), "sample_stationary_stacks": c.ss}
            f.write(json.dumps(rec) + "\n")
            print(json.dumps(rec))
        rec = mix_alone(args.batch, args.mix_reps)
        f.write(json.dumps(rec) + "\n")
        print(json.dumps(rec))


if __name__ == "__main__":
    main()
