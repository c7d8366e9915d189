"""Cost of the encoder's options (temporal 'embedding', aggregation 'max', do_norm) at cfg-B (d 512, 2 + 2 layers, V 30522, batch 256,
captions of 20 tokens): the training step of the default `mme` block and of each single option (and all three) at the same shape.

    python tools/bench_encoder_variants.py [--steps 30] [--warmup 8] [--rounds 3] [--out profiles/encoder_variants_bench.jsonl]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o ev -- python tools/bench_encoder_variants.py --trace-only CASE
    python tools/bench_encoder_variants.py --summarize DIR --case CASE [--out FILE]   # front-end kernel times + bytes -> one JSON line

One stream [512] with T 12 (bench.py's headline shape) and two streams [512, 128] with T (12, 4) (tools/bench_multimodal.py's).  All
cases live in one process and are measured in alternating rounds (a round runs every case once), so a ratio compares neighbours in
time, not two processes.  Per case one JSON line: ms/step per round and their median (CaptionTrainer, launch list, FusedAdam:
bench.py's executor), the ratio to the default case of the same stream count, the default's own spread over the rounds, and which
stacks ran sample-stationary.  With one stream the default runs the front end inside the sample-stationary kernel's prologue; a
variant replaces that by the input cast, the unify GEMM and one vct_enc_frontend_ex_fwd launch (and by the backward launch(es) in
place of vct_enc_frontend_bwd)."""
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

OPTS = {"default": {}, "embedding": {"temporal": "embedding"}, "max": {"aggregation": "max"}, "norm": {"do_norm": True},
        "all": {"temporal": "embedding", "aggregation": "max", "do_norm": True}}
STREAMS = {"one": ([512], (12,)), "two": ([512, 128], (12, 4))}
CASES = [(f"{s}_{o}", s, o) for s in STREAMS for o in OPTS]
HBM_GBPS = bench.PEAK_HBM_GBS      # the HBM3E figure bench.py's roofline lines use


def model_for(shapes, opts):
    from vct_amd.model import MMT4Caption
    mc = copy.deepcopy(bench.MODEL_CFG)
    mc["modal"] = [f"m{i}" for i in range(len(shapes))]
    mc["modal_shape"] = list(shapes)
    mc["video_encoder"]["mme"].update(opts)
    torch.manual_seed(666)
    m = MMT4Caption(mc, device=torch.device("cuda"), compute_dtype=torch.bfloat16)
    m.mode("caption")
    return m


class Case:
    def __init__(self, name, streams, opt, B):
        from vct_amd import engine
        from vct_amd.trainer import CaptionTrainer, build_optimizer
        self.name, self.streams, self.opt = name, streams, opt
        shapes, Ts = STREAMS[streams]
        self.model = model_for(shapes, OPTS[opt])
        self.model.train()
        o, _ = build_optimizer(bench.TRAIN_CFG, self.model)
        self.trainer = CaptionTrainer(self.model, o, None, use_graph=False, launch_list=True)
        self.inputs = self.trainer.adopt_inputs(*batch_for(shapes, Ts, B))
        seen, orig = [], engine._StackBase._stack_ss

        def spy(eng, *a, **k):
            seen.append(type(eng).__name__)
            return orig(eng, *a, **k)
        engine._StackBase._stack_ss = spy
        try:
            self.trainer.step(*self.inputs)          # eager first step (allocates), records which stacks were fused
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


def frontend_bytes(kind, B, Ts, opts, d=512):
    """Bytes the vct_enc_frontend_ex kernels request (bf16 activations).  Forward: the unify outputs read (2 B x rows; the aggregation
    row's second pass over them hits in the cache and is not counted) + the frame masks, the stack input and key-pad bytes written,
    the fp32 temporal / modal rows, and with the norm its two vectors and the two statistics per row.  Backward without the norm:
    d(stack input) read by the row workgroups and again by the parameter sums when there are any, the unify outputs under 'max', du
    written, the fp32 parameter gradients written (all 512 rows of the embedding table).  With the norm: d(stack input) and the unify
    outputs read, dpre written in fp32 and read back by du and by the sums, the norm partials written."""
    S, T, n = sum(t + 1 for t in Ts), sum(Ts), len(Ts)
    learned, by_max, norm = opts.get("temporal") == "embedding", opts.get("aggregation") == "max", bool(opts.get("do_norm"))
    n_labels = 2 * n if n > 1 else 0
    if kind == "fwd":
        return 2 * B * T * d + B * T + 2 * B * S * d + B * S + 4 * (S + n_labels) * d + (8 * d + 8 * B * S if norm else 0)
    sums = n_labels > 0 or learned
    grads = 4 * n_labels * d + (4 * 512 * d if learned else 0)
    if not norm:
        return 2 * B * S * d * (2 if sums else 1) + (2 * B * T * d if by_max else 0) + 2 * B * T * d + grads
    return 2 * B * S * d + 2 * B * T * d + 4 * B * S * d * (3 if sums else 2) + 2 * B * T * d + 8 * B * n * d + grads


def summarize(trace_dir, case, batch, out):
    import csv
    import glob
    _, streams, opt = next(c for c in CASES if c[0] == case)
    Ts = STREAMS[streams][1]
    paths = glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True)
    if not paths:
        raise SystemExit(f"no kernel_stats.csv under {trace_dir}")
    res = {"record": "frontend_kernels", "case": case, "batch": batch, "T": list(Ts), "S": sum(t + 1 for t in Ts), "kernels": {}}
    with open(paths[0]) as f:
        for r in csv.DictReader(f):
            for kind in ("fwd", "bwd"):
                if f"enc_frontend_ex_{kind}_kernel" in r["Name"]:
                    nbytes = frontend_bytes(kind, batch, Ts, OPTS[opt])
                    calls, total = int(r["Calls"]), float(r["TotalDurationNs"]) / 1e3
                    per_step = 2 if kind == "bwd" and OPTS[opt].get("do_norm") and (len(Ts) > 1 or OPTS[opt].get("temporal") == "embedding") else 1
                    us = total / calls * per_step           # the backward's two launches (rows, then sums) count as one pass
                    res["kernels"][kind] = {"calls": calls, "launches_per_step": per_step, "us_per_step": round(us, 2),
                                            "min_us_one_launch": round(float(r["MinNs"]) / 1e3, 2), "bytes_requested": nbytes,
                                            "GBps": round(nbytes / (us * 1e-6) / 1e9, 1),
                                            "frac_of_hbm_peak": round(nbytes / (us * 1e-6) / 1e9 / HBM_GBPS, 4)}
    line = json.dumps(res)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")
    print(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--out", default=None, help="JSON lines (default profiles/encoder_variants_bench.jsonl; --summarize: appended to)")
    ap.add_argument("--trace-only", metavar="CASE", help="a few steps of one case (for rocprofv3 --kernel-trace --stats)")
    ap.add_argument("--summarize", metavar="DIR", help="reduce the rocprofv3 --stats output of a --trace-only run")
    ap.add_argument("--case", help="--summarize: the case that run traced")
    args = ap.parse_args()
    if args.summarize:
        summarize(args.summarize, args.case, args.batch, args.out)
        return
    if args.trace_only:
        _, s, o = next(c for c in CASES if c[0] == args.trace_only)
        Case(args.trace_only, s, o, args.batch).run(5, 2)
        return
    cases = [Case(n, s, o, args.batch) for n, s, o in CASES]
    for _ in range(args.rounds):
        for c in cases:
            c.run(args.steps, args.warmup)
    med = {c.name: sorted(c.times)[len(c.times) // 2] for c in cases}
    out = args.out or os.path.join(ROOT, "profiles", "encoder_variants_bench.jsonl")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        for c in cases:
            base = next(b for b in cases if b.streams == c.streams and b.opt == "default")
            rec = {"record": "train_step", "case": c.name, "streams": c.streams, "options": OPTS[c.opt], "batch": args.batch,
                   "modal_shape": STREAMS[c.streams][0], "T": list(STREAMS[c.streams][1]), "steps": args.steps, "rounds": args.rounds,
                   "ms_per_step_rounds": [round(t, 4) for t in c.times], "ms_per_step_median": round(med[c.name], 4),
                   "over_default": round(med[c.name] / med[base.name], 4),
                   "default_spread": round((max(base.times) - min(base.times)) / med[base.name], 4),
                   "sample_stationary_stacks": c.ss}
            f.write(json.dumps(rec) + "\n")
            print(json.dumps(rec))


if __name__ == "__main__":
    main()
