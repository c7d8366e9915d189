#!/usr/bin/env python
"""Sampled-decode benchmark: cfg-B model (bench.MODEL_CFG) in eval mode, bf16, synthetic (B, 12, 512) features, max_len 30,
(videos, samples) in {(16, 5), (128, 1)}: 80 and 128 rows.  ONE sampling session per shape serves every setting (the kernels
read them from the device control block); per setting -- k = 0, k = 5, k = 64 with p = 0.9 -- one JSON line:
  * us_per_step_sample: one token step of the sampling session (its captured graph per position, replayed back to back over
    t = 1..29: the decode step of the rows + vct_sample_select), median over the rounds;
  * us_per_step_greedy: the same for a greedy session of the same row count in the same process, rounds alternating with the
    sampling session's; greedy_spread = (max - min) / median of the greedy rounds, the noise floor beside the ratio;
  * sample_over_greedy: the ratio of the medians.
--out FILE appends the lines to FILE (profiles/sample_bench.jsonl).  The two kernels' own time comes from a separate profiler run:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o sample -- python tools/bench_sample.py --quick --shape 16,5 --setting 5,1.0
    python tools/bench_sample.py --summarize OUT      (per-kernel lines of the stats CSV as JSON)"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import MODEL_CFG  # noqa: E402

SHAPES = ((16, 5), (128, 1))
SETTINGS = ((0, 1.0), (5, 1.0), (64, 0.9))        # (top_k, top_p) at temperature 1
MAX_LEN = 30


def _step_us(st, reps):
    """Reset the session (its begin graph), then replay its per-position graphs t = 1..MAX_LEN-1 `reps` times; device time per step."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = sorted(st.graphs)
    st.begin["g"].replay()
    e0.record()
    for _ in range(reps):
        for t in ts:
            st.graphs[t].replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (reps * len(ts))


def run(quick: bool, shapes=SHAPES, out=None, settings=SETTINGS):
    from vct_amd import decode
    from vct_amd.model import MMT4Caption
    dev = torch.device("cuda", 0)
    torch.manual_seed(666)
    reps, rounds = (1, 1) if quick else (10, 7)
    dtype = torch.bfloat16
    m = MMT4Caption(MODEL_CFG, device=dev, compute_dtype=dtype)
    m.mode("caption")
    m.eval()
    for B, N in shapes:
        feats = torch.randn(B, 12, 512, generator=torch.Generator().manual_seed(0)).to(dev)
        feats_g = feats.repeat_interleave(N, 0)
        # lookahead past the end: every session captures all MAX_LEN - 1 positions (random weights rarely emit [SEP])
        for _ in range(2):
            decode.sample_decode_ids(m, feats, None, max_len=MAX_LEN, num_samples=N, seed=1, lookahead=MAX_LEN)
            decode.greedy_decode_ids(m, feats_g, None, max_len=MAX_LEN, lookahead=MAX_LEN)
        torch.cuda.synchronize()
        sessions = m.__dict__["_decode_sessions"]
        st_s = sessions[("sample", B, N, 13, MAX_LEN, dtype)]
        st_g = sessions[(B * N, 13, MAX_LEN, dtype)]
        for top_k, top_p in settings:
            st_s.set_sampling(1, top_k, 1.0, top_p)
            us_s, us_g = [], []
            for _ in range(rounds):                       # rounds alternate between the two sessions
                us_s.append(_step_us(st_s, reps))
                us_g.append(_step_us(st_g, reps))
            ms, mg = statistics.median(us_s), statistics.median(us_g)
            line = json.dumps({"bench": "sample_decode", "dtype": "bfloat16", "videos": B, "samples": N, "rows": B * N,
                               "top_k": top_k, "top_p": top_p, "temperature": 1.0, "rounds": rounds, "reps": reps,
                               "steps_captured": len(st_s.graphs), "us_per_step_sample": round(ms, 1),
                               "us_per_step_greedy": round(mg, 1), "sample_over_greedy": round(ms / mg, 3),
                               "greedy_spread": round((max(us_g) - min(us_g)) / mg, 3),
                               "sample_spread": round((max(us_s) - min(us_s)) / ms, 3)})
            print(line, flush=True)
            if out:
                with open(out, "a") as f:
                    f.write(line + "\n")


def summarize(out_dir):
    paths = glob.glob(os.path.join(out_dir, "**", "*kernel_stats.csv"), recursive=True)
    if not paths:
        raise SystemExit(f"no kernel_stats.csv under {out_dir}")
    with open(paths[0]) as f:
        for r in csv.DictReader(f):
            name = r["Name"]
            if "sample_" not in name and "argmax_rows" not in name:
                continue
            print(json.dumps({"kernel": name.split("(")[0].replace("void ", "").replace("vct::", ""), "calls": int(r["Calls"]),
                              "avg_us": round(float(r["AverageNs"]) / 1e3, 2), "min_us": round(float(r["MinNs"]) / 1e3, 2),
                              "max_us": round(float(r["MaxNs"]) / 1e3, 2)}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="one pass per configuration (for the profiler run)")
    ap.add_argument("--shape", metavar="B,N", help="one (videos, samples) configuration instead of both")
    ap.add_argument("--setting", metavar="K,P", help="one (top_k, top_p) setting instead of all three (for the profiler run)")
    ap.add_argument("--out", metavar="FILE", help="append the JSON lines to FILE")
    ap.add_argument("--summarize", metavar="DIR", help="print the sampling kernels of a rocprofv3 --stats run")
    a = ap.parse_args()
    if a.summarize:
        summarize(a.summarize)
    else:
        settings = ((int(a.setting.split(",")[0]), float(a.setting.split(",")[1])),) if a.setting else SETTINGS
        run(a.quick, (tuple(int(v) for v in a.shape.split(",")),) if a.shape else SHAPES, a.out, settings)
