#!/usr/bin/env python
"""Beam-search decode benchmark: cfg-B model (bench.MODEL_CFG) in eval mode, synthetic (B, 12, 512) features, max_len 30,
bf16 and fp32, (B, K) in {(1, 5), (16, 5), (64, 4)}.  Prints one JSON line per configuration:
  * us_per_step_beam: one token step of the beam session (its captured graph per position, replayed back to back over
    t = 1..29: the decode step of B*K rows + vct_beam_select + vct_beam_reorder);
  * us_per_step_greedy: the same for a greedy session at batch B*K (same step, greedy selection);
  * ms_per_decode_beam: a whole beam_decode_ids call (begin graph, steps, stop polling, back-tracking).
Kernel times of the two beam kernels come from a separate profiler run of this script with --quick:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o beam -- python tools/bench_beam.py --quick --shape 16,5 --dtype bf16
    python tools/bench_beam.py --summarize OUT      (per-kernel lines of the stats CSV as JSON)"""
import argparse
import csv
import glob
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import MODEL_CFG  # noqa: E402

SHAPES = ((1, 5), (16, 5), (64, 4))
MAX_LEN = 30


def _step_us(st, reps):
    """Replay the session's per-position graphs t = 1..MAX_LEN-1 `reps` times; device time per step."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = sorted(st.graphs)
    e0.record()
    for _ in range(reps):
        for t in ts:
            st.graphs[t].replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (reps * len(ts))


def run(quick: bool, shapes=SHAPES, dtypes=(torch.bfloat16, torch.float32)):
    from vct_amd import decode
    from vct_amd.model import MMT4Caption
    dev = torch.device("cuda", 0)
    torch.manual_seed(666)
    reps = 1 if quick else 20
    for dtype in dtypes:
        m = MMT4Caption(MODEL_CFG, device=dev, compute_dtype=dtype)
        m.mode("caption")
        m.eval()
        for B, K in shapes:
            feats = torch.randn(B, 12, 512, generator=torch.Generator().manual_seed(0)).to(dev)
            feats_g = feats.repeat_interleave(K, 0)
            # lookahead past the end: every session captures all MAX_LEN - 1 positions (random weights rarely emit [SEP])
            for _ in range(2):
                ids = decode.beam_decode_ids(m, feats, None, K, max_len=MAX_LEN, lookahead=MAX_LEN)
                decode.greedy_decode_ids(m, feats_g, None, max_len=MAX_LEN, lookahead=MAX_LEN)
            torch.cuda.synchronize()
            sessions = m.__dict__["_decode_sessions"]
            st_b = sessions[("beam", B, K, 13, MAX_LEN, dtype)]
            st_g = sessions[(B * K, 13, MAX_LEN, dtype)]
            us_b = _step_us(st_b, reps)
            us_g = _step_us(st_g, reps)
            n = 2 if quick else 10
            t0 = time.perf_counter()
            for _ in range(n):
                ids = decode.beam_decode_ids(m, feats, None, K, max_len=MAX_LEN)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) / n * 1e3
            print(json.dumps({"bench": "beam_decode", "dtype": str(dtype).split(".")[-1], "videos": B, "beams": K, "rows": B * K,
                              "steps_captured": len(st_b.graphs), "ids_len": ids.shape[1],
                              "us_per_step_beam": round(us_b, 1), "us_per_step_greedy": round(us_g, 1),
                              "beam_over_greedy": round(us_b / us_g, 3), "ms_per_decode_beam": round(ms, 3)}), flush=True)


def summarize(out_dir):
    paths = glob.glob(os.path.join(out_dir, "**", "*kernel_stats.csv"), recursive=True)
    if not paths:
        raise SystemExit(f"no kernel_stats.csv under {out_dir}")
    with open(paths[0]) as f:
        for r in csv.DictReader(f):
            name = r["Name"]
            if "beam_" not in name and "argmax_rows" not in name:
                continue
            print(json.dumps({"kernel": name.split("(")[0].replace("void ", "").replace("vct::", ""), "calls": int(r["Calls"]),
                              "avg_us": round(float(r["AverageNs"]) / 1e3, 2), "min_us": round(float(r["MinNs"]) / 1e3, 2),
                              "max_us": round(float(r["MaxNs"]) / 1e3, 2)}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="one pass per configuration (for the profiler run)")
    ap.add_argument("--shape", metavar="B,K", help="one (videos, beams) configuration instead of all three")
    ap.add_argument("--dtype", choices=("bf16", "fp32"), help="one compute dtype instead of both")
    ap.add_argument("--summarize", metavar="DIR", help="print the beam kernels of a rocprofv3 --stats run")
    a = ap.parse_args()
    if a.summarize:
        summarize(a.summarize)
    else:
        shapes = (tuple(int(v) for v in a.shape.split(",")),) if a.shape else SHAPES
        dtypes = ({"bf16": torch.bfloat16, "fp32": torch.float32}[a.dtype],) if a.dtype else (torch.bfloat16, torch.float32)
        run(a.quick, shapes, dtypes)
