#!/usr/bin/env python
"""Generation-controls benchmark: cfg-B model (bench.MODEL_CFG) in eval mode, bf16, synthetic (B, 12, 512) features, max_len 30.
Four session shapes -- greedy at batch 1 and batch 128, 16 videos x 5 beams, 64 videos x 5 samples -- each decoded twice in ONE
process: without controls and with GenerationControls(min_length=5, no_repeat_ngram_size=3, repetition_penalty=1.2).  Per shape one
JSON line:
  * us_per_step_plain / us_per_step_controls: one token step of the session (its captured graph per position, replayed back to
    back over t = 1..29), median over rounds that alternate between the two sessions, timed between stream events;
  * added_us = the difference of the medians (the structure says one more dependent launch, vct_logit_controls, per step);
    plain_spread = (max - min) / median of the plain rounds, the noise floor beside it;
  * variant_plain / variant_controls: the decode step each session takes (batch-1 greedy leaves the block step for the gemv step
    when controls are on, so that line compares two different steps).
--out FILE appends the lines to FILE (profiles/gen_controls_bench.jsonl)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import MODEL_CFG  # noqa: E402

MAX_LEN = 30
SHAPES = (("greedy", 1, 1), ("greedy", 128, 1), ("beam", 16, 5), ("sample", 64, 5))       # (decoder, videos, beams / samples)


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


def run(quick: bool, out=None, shapes=SHAPES):
    from vct_amd import decode, engine
    from vct_amd.model import MMT4Caption
    dev = torch.device("cuda", 0)
    torch.manual_seed(666)
    reps, rounds = (1, 1) if quick else (10, 7)
    dtype = torch.bfloat16
    m = MMT4Caption(MODEL_CFG, device=dev, compute_dtype=dtype)
    m.mode("caption")
    m.eval()
    eng = m.cap_decoder._engine()
    controls = decode.GenerationControls(min_length=5, no_repeat_ngram_size=3, repetition_penalty=1.2)
    for kind, B, N in shapes:
        feats = torch.randn(B, 12, 512, generator=torch.Generator().manual_seed(0)).to(dev)
        m.__dict__.pop("_decode_sessions", None)             # two sessions per shape; the cache holds four
        # lookahead past the end: every session captures all MAX_LEN - 1 positions
        for c in (None, controls, None, controls):
            if kind == "greedy":
                decode.greedy_decode_ids(m, feats, None, max_len=MAX_LEN, lookahead=MAX_LEN, controls=c)
            elif kind == "beam":
                decode.beam_decode_ids(m, feats, None, N, max_len=MAX_LEN, lookahead=MAX_LEN, controls=c)
            else:
                decode.sample_decode_ids(m, feats, None, max_len=MAX_LEN, num_samples=N, top_k=5, seed=1, lookahead=MAX_LEN, controls=c)
        torch.cuda.synchronize()
        sessions = m.__dict__["_decode_sessions"]
        (st_c,) = [st for k, st in sessions.items() if "ctl" in k]
        (st_p,) = [st for k, st in sessions.items() if "ctl" not in k]
        us_p, us_c = [], []
        for _ in range(rounds):                                # rounds alternate between the two sessions
            us_p.append(_step_us(st_p, reps))
            us_c.append(_step_us(st_c, reps))
        mp, mc = statistics.median(us_p), statistics.median(us_c)
        line = json.dumps({"bench": "gen_controls", "dtype": "bfloat16", "decoder": kind, "videos": B, "per_video": N, "rows": B * N,
                           "min_length": 5, "no_repeat_ngram_size": 3, "repetition_penalty": 1.2, "rounds": rounds, "reps": reps,
                           "steps_captured": [len(st_p.graphs), len(st_c.graphs)],
                           "variant_plain": engine.decode_step_variant(eng, st_p),
                           "variant_controls": engine.decode_step_variant(eng, st_c),
                           "us_per_step_plain": round(mp, 1), "us_per_step_controls": round(mc, 1), "added_us": round(mc - mp, 1),
                           "plain_spread": round((max(us_p) - min(us_p)) / mp, 3),
                           "controls_spread": round((max(us_c) - min(us_c)) / mc, 3)})
        print(line, flush=True)
        if out:
            with open(out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="one pass per shape")
    ap.add_argument("--out", metavar="FILE", help="append the JSON lines to FILE")
    a = ap.parse_args()
    run(a.quick, a.out)
