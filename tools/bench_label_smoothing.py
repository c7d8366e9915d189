#!/usr/bin/env python
"""Label-smoothing benchmark on BASELINE.json configs[1] (bench.MODEL_CFG, bf16, batch 256).  Every figure is the median of --rounds (9)
measurements between stream events, the cases alternating inside a round, all in one process:

  {"bench": "label_smoothing_loss"}: us per loss call (count + row kernel + finalise) on 4864 rows x 30522 logits, bf16, in place, of
    sce        ops.sce_loss (vct_sce_loss), the shipped path;
    ls_eps0    ops.sce_loss_ls at smoothing 0 with the statistics;
    ls_eps01   ops.sce_loss_ls at smoothing 0.1 with the statistics;
    wce        ops.wce_loss (vct_wce_loss) with a random device seq_w and tok_logp.
    Each case owns its logits buffer, refilled with the same random logits before every measurement (a call overwrites it with the
    gradient).
  {"bench": "label_smoothing_step"}: ms per training step on the recorded launch list, dropout on, --steps steps per measurement, of
    absent     the configuration as shipped (no caption_decoder.label_smoothing key: the ops.sce_loss call);
    eps01      caption_decoder.label_smoothing = 0.1.
--only loss|step runs one of the two; --absent-only leaves the eps01 case out of the step benchmark; --label TEXT is copied into the
lines.  An A/B of two checkouts runs `--only step --absent-only` in both (a tree without the feature reports `absent` alone anyway):
one model in the process on either side.  --out FILE appends the lines (profiles/label_smoothing_bench.jsonl)."""
import argparse
import copy
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import MODEL_CFG, synthetic  # noqa: E402


def _events(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def _summary(t, digits):
    med = statistics.median
    return ({k: round(med(v), digits) for k, v in t.items()},
            {k: round((max(v) - min(v)) / med(v), 3) for k, v in t.items()})


def bench_loss(batch, calls, rounds, alpha):
    from vct_amd import ops
    dev = torch.device("cuda", 0)
    S, V = 20, 30522
    N, Vp = batch * (S - 1), (V + 31) // 32 * 32
    g = torch.Generator(device=dev).manual_seed(1)
    src = (3.0 * torch.randn(N, Vp, device=dev, generator=g)).to(torch.bfloat16)
    ids = torch.randint(3, V, (batch, S), device=dev, generator=g)
    ids[::3, S - 4:] = 0                                            # pad tails
    loss, stats = torch.zeros(1, device=dev), torch.zeros(2, device=dev)
    ws = torch.zeros(4 * N + 2, device=dev)
    seq_w, tok_logp = torch.randn(batch, device=dev, generator=g), torch.zeros(N, device=dev)
    bufs = {k: torch.empty_like(src) for k in ("sce", "ls_eps0", "ls_eps01", "wce")}
    fns = {"sce": lambda: ops.sce_loss(bufs["sce"], V, ids[:, 1:], S - 1, 0, alpha, loss, bufs["sce"], ws),
           "ls_eps0": lambda: ops.sce_loss_ls(bufs["ls_eps0"], V, ids[:, 1:], S - 1, 0, alpha, 0.0, loss, bufs["ls_eps0"], ws, stats=stats),
           "ls_eps01": lambda: ops.sce_loss_ls(bufs["ls_eps01"], V, ids[:, 1:], S - 1, 0, alpha, 0.1, loss, bufs["ls_eps01"], ws, stats=stats),
           "wce": lambda: ops.wce_loss(bufs["wce"], V, ids[:, 1:], S - 1, 0, seq_w, loss, bufs["wce"], ws, tok_logp=tok_logp)}
    for k, fn in fns.items():
        bufs[k].copy_(src)
        _events(fn, 3)
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            bufs[k].copy_(src)
            t[k].append(_events(fn, calls) * 1e3)
    us, spread = _summary(t, 2)
    return {"bench": "label_smoothing_loss", "dtype": "bfloat16", "rows": N, "V": V, "ld": Vp, "alpha": alpha, "in_place": True,
            "calls": calls, "rounds": rounds, "us": us, "spread": spread,
            "ls_eps0_minus_sce_us": round(us["ls_eps0"] - us["sce"], 2), "ls_eps01_minus_sce_us": round(us["ls_eps01"] - us["sce"], 2),
            "bytes_per_call": 2 * N * Vp * 2, "sce_GBps": round(2 * N * Vp * 2 / us["sce"] / 1e3, 1),
            "ls_eps01_GBps": round(2 * N * Vp * 2 / us["ls_eps01"] / 1e3, 1)}


def bench_step(batch, steps, rounds, warmup, with_eps=True):
    from vct_amd.model import MMT4Caption
    from vct_amd.trainer import CaptionTrainer, FusedAdam
    dev = torch.device("cuda", 0)

    def trainer(eps=None):
        torch.manual_seed(666)
        mc = copy.deepcopy(MODEL_CFG)
        if eps is not None:
            mc["caption_decoder"]["label_smoothing"] = eps
        m = MMT4Caption(mc, device=dev, compute_dtype=torch.bfloat16)
        m.mode("caption")
        m.train()
        tr = CaptionTrainer(m, FusedAdam(m, lr=1e-4), launch_list=True)
        data = tr.adopt_inputs(*synthetic(batch, 0, dev))
        for _ in range(warmup):
            tr.step(*data)
        torch.cuda.synchronize()
        return tr, data

    cases = {"absent": trainer()}
    if with_eps:
        cases["eps01"] = trainer(0.1)
        assert cases["eps01"][0].last_nll is not None and cases["absent"][0].last_nll is None
    t = {k: [] for k in cases}
    for _ in range(rounds):
        for k, (tr, data) in cases.items():
            t[k].append(_events(lambda: tr.step(*data), steps))
    ms, spread = _summary(t, 4)
    line = {"bench": "label_smoothing_step", "dtype": "bfloat16", "batch": batch, "executor": "list", "steps": steps, "rounds": rounds,
            "step_ms": ms, "spread": spread, "rounds_ms": {k: [round(x, 4) for x in v] for k, v in t.items()}}
    if with_eps:
        line["eps01_minus_absent_ms"] = round(ms["eps01"] - ms["absent"], 4)
    return line


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20, help="training steps per measurement")
    ap.add_argument("--calls", type=int, default=20, help="loss calls per measurement")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--alpha", type=float, default=float(MODEL_CFG["caption_decoder"]["sce_loss_alpha"]))
    ap.add_argument("--only", choices=("loss", "step"))
    ap.add_argument("--absent-only", action="store_true", help="step benchmark: the shipped configuration alone")
    ap.add_argument("--label", help="copied into every line")
    ap.add_argument("--out", metavar="FILE", help="append the JSON lines to FILE")
    a = ap.parse_args()
    from vct_amd import ops as _ops
    have = hasattr(_ops, "sce_loss_ls")
    lines = []
    if a.only != "step":
        lines.append(bench_loss(a.batch, a.calls, a.rounds, a.alpha))
    if a.only != "loss":
        lines.append(bench_step(a.batch, a.steps, a.rounds, a.warmup, with_eps=have and not a.absent_only))
    for line in lines:
        if a.label:
            line["label"] = a.label
        s = json.dumps(line)
        print(s, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(s + "\n")
