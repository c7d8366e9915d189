#!/usr/bin/env python
"""Ensemble-decoding benchmark: cfg-B models (bench.MODEL_CFG, one seed per member) in eval mode, bf16, synthetic (B, 12, 512)
features, max_len 30.  Every figure is the median of --rounds (9) measurements between stream events, the cases alternating
inside a round.

  {"bench": "ensemble_step"}, one line per session shape (greedy at batch 128; 16 videos x 5 beams): us per token step (the
    captured graph per position, replayed back to back over t = 1..29) of the plain single-model session (members 1) and of
    decode.Ensemble over 2, 3 and 4 members of the same shape, mode "prob"; per_member_us = (ensemble - plain) / (M - 1).
  {"bench": "ensemble_combine"}: us per call of ops.ensemble_combine alone at V = 30522, 128 rows, bf16 members in ONE buffer,
    both modes, for 2 and 4 members -- beside ops.warm over the same member bytes (the read-only pass: same bytes, no
    arithmetic, no fp32 output row).
--out FILE appends the lines (profiles/ensemble_bench.jsonl)."""
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
SHAPES = (("greedy", 128, 1), ("beam", 16, 5))       # (decoder, videos, beams)
MEMBERS = (1, 2, 3, 4)


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


def _call_us(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def _emit(line, out):
    s = json.dumps(line)
    print(s, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(s + "\n")


def run(rounds, reps, calls, out=None):
    from vct_amd import decode, ops
    from vct_amd.model import MMT4Caption
    dev = torch.device("cuda", 0)
    med = statistics.median
    models = []
    for seed in range(max(MEMBERS)):
        torch.manual_seed(666 + seed)
        m = MMT4Caption(MODEL_CFG, device=dev, compute_dtype=torch.bfloat16)
        m.mode("caption")
        m.eval()
        models.append(m)
    for kind, B, K in SHAPES:
        feats = torch.randn(B, 12, 512, generator=torch.Generator().manual_seed(0)).to(dev)
        sessions = {}
        for M in MEMBERS:
            # lookahead past the end: every session captures all MAX_LEN - 1 positions
            owner = models[0] if M == 1 else decode.Ensemble(models[:M])
            owner.__dict__.pop("_decode_sessions", None)
            for _ in range(2):
                if M == 1 and kind == "greedy":
                    decode.greedy_decode_ids(owner, feats, None, max_len=MAX_LEN, lookahead=MAX_LEN)
                elif M == 1:
                    decode.beam_decode_ids(owner, feats, None, K, max_len=MAX_LEN, lookahead=MAX_LEN)
                elif kind == "greedy":
                    owner.greedy_decode_ids(feats, None, max_len=MAX_LEN, lookahead=MAX_LEN)
                else:
                    owner.beam_decode_ids(feats, None, K, max_len=MAX_LEN, lookahead=MAX_LEN)
            torch.cuda.synchronize()
            (sessions[M],) = owner.__dict__["_decode_sessions"].values()
            sessions[M].owner = owner                            # (keeps an Ensemble and its weight block alive)
        us = {M: [] for M in MEMBERS}
        for _ in range(rounds):
            for M in MEMBERS:
                us[M].append(_step_us(sessions[M], reps))
        m_us = {M: med(v) for M, v in us.items()}
        _emit({"bench": "ensemble_step", "dtype": "bfloat16", "decoder": kind, "videos": B, "per_video": K, "rows": B * K, "mode": "prob",
               "rounds": rounds, "reps": reps, "steps_captured": {str(M): len(sessions[M].graphs) for M in MEMBERS},
               "us_per_step": {str(M): round(m_us[M], 1) for M in MEMBERS},
               "over_plain": {str(M): round(m_us[M] / m_us[1], 3) for M in MEMBERS if M > 1},
               "per_member_us": {str(M): round((m_us[M] - m_us[1]) / (M - 1), 1) for M in MEMBERS if M > 1},
               "spread": {str(M): round((max(v) - min(v)) / med(v), 3) for M, v in us.items()}}, out)
        del sessions

    # the combine launch alone
    rows, V = 128, 30522
    Vp = (V + 31) // 32 * 32
    for M in (2, 4):
        buf = torch.randn(M, rows, Vp, generator=torch.Generator().manual_seed(M)).to(dev, torch.bfloat16)
        xs = [buf[m] for m in range(M)]
        w = torch.tensor([1.0 / M] * M + [0.0] * (8 - M), dtype=torch.float32, device=dev)
        o = torch.empty(rows, Vp, dtype=torch.float32, device=dev)
        fns = {"prob": lambda: ops.ensemble_combine(xs, w, o, "prob", cols=V), "logp": lambda: ops.ensemble_combine(xs, w, o, "logp", cols=V),
               "warm": lambda: ops.warm(buf)}
        for fn in fns.values():
            _call_us(fn, 3)
        u = {k: [] for k in fns}
        for _ in range(rounds):
            for k, fn in fns.items():
                u[k].append(_call_us(fn, calls))
        t = {k: med(v) for k, v in u.items()}
        nbytes = buf.numel() * 2
        _emit({"bench": "ensemble_combine", "rows": rows, "V": V, "members": M, "member_dtype": "bfloat16", "member_bytes": nbytes,
               "out_bytes": rows * V * 4, "calls": calls, "rounds": rounds, "us": {k: round(v, 2) for k, v in t.items()},
               "spread": {k: round((max(v) - min(v)) / med(v), 3) for k, v in u.items()},
               "prob_over_warm": round(t["prob"] / t["warm"], 3), "logp_over_warm": round(t["logp"] / t["warm"], 3),
               "warm_GBps": round(nbytes / t["warm"] / 1e3, 1)}, out)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=5, help="passes over the 29 step graphs per measurement")
    ap.add_argument("--calls", type=int, default=20, help="combine launches per measurement")
    ap.add_argument("--out", metavar="FILE", help="append the JSON lines to FILE")
    a = ap.parse_args()
    run(a.rounds, a.reps, a.calls, a.out)
