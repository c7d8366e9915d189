#!/usr/bin/env python
"""Gradient-clipping benchmark on BASELINE.json configs[1] (bench.MODEL_CFG, bf16, batch 256, recorded launch list, dropout on).
Two JSON lines, every figure the median of --rounds (9) measurements between stream events, the cases alternating inside a round:

  {"bench": "grad_clip_step"}: ms per training step, --steps steps per measurement, of
    (a) fused      the step as shipped (optimizer inside the weight-gradient GEMMs);
    (b) unfused    the same step with the fusion off (VCT_FUSE_ADAM=0): what a user of torch's clip_grad_norm_ had to run;
    (c) clip_idle  max_grad_norm = 1e9: the norm is measured, the coefficient is 1, the scaling launch leaves at once;
    (d) clip_on    max_grad_norm = half the measured norm: every gradient is scaled.
    (c) - (b) is the price of the feature, (b) - (a) the known price of leaving the fusion.
  {"bench": "grad_clip_norm_pass"}: us per call, --calls calls per measurement, on the gradient buffer of the same model, of
    sqnorm   ops.grad_sqnorm (two launches: fp64 partials, then the finish);
    warm     ops.warm over the same byte range (the read-only pass of the parent: same bytes, no arithmetic);
    apply_on / apply_idle   ops.grad_clip_apply with coef < 1 / coef == 1.
--out FILE appends both lines (profiles/grad_clip_bench.jsonl)."""
import argparse
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


def run(batch, steps, calls, rounds, warmup, out=None):
    from vct_amd import ops
    from vct_amd.model import MMT4Caption
    from vct_amd.trainer import CaptionTrainer, FusedAdam
    dev = torch.device("cuda", 0)

    def trainer(fuse=True, **clip):
        torch.manual_seed(666)
        m = MMT4Caption(MODEL_CFG, device=dev, compute_dtype=torch.bfloat16)
        m.mode("caption")
        m.train()
        was = FusedAdam.fuse_dw_default
        FusedAdam.fuse_dw_default = bool(fuse) and was
        try:
            tr = CaptionTrainer(m, FusedAdam(m, lr=1e-4, **clip), launch_list=True)
        finally:
            FusedAdam.fuse_dw_default = was
        data = tr.adopt_inputs(*synthetic(batch, 0, dev))
        for _ in range(warmup):
            tr.step(*data)
        torch.cuda.synchronize()
        return tr, data

    cases = {"fused": trainer(), "unfused": trainer(fuse=False), "clip_idle": trainer(max_grad_norm=1e9)}
    idle = cases["clip_idle"][0]
    norm = float(idle.last_grad_norm)
    cases["clip_on"] = trainer(max_grad_norm=0.5 * norm)
    assert cases["fused"][0].fuse_adam and not cases["unfused"][0].fuse_adam and not idle.fuse_adam
    t = {k: [] for k in cases}
    for _ in range(rounds):
        for k, (tr, data) in cases.items():
            t[k].append(_events(lambda: tr.step(*data), steps))
    med = statistics.median
    coef_on = float(cases["clip_on"][0].last_clip_coef)
    assert float(idle.last_clip_coef) == 1.0 and 0.0 < coef_on < 1.0
    ms = {k: round(med(v), 4) for k, v in t.items()}
    lines = [{"bench": "grad_clip_step", "dtype": "bfloat16", "batch": batch, "executor": "list", "steps": steps, "rounds": rounds,
              "step_ms": ms, "spread": {k: round((max(v) - min(v)) / med(v), 3) for k, v in t.items()},
              "clip_idle_minus_unfused_ms": round(ms["clip_idle"] - ms["unfused"], 4),
              "clip_on_minus_unfused_ms": round(ms["clip_on"] - ms["unfused"], 4),
              "unfused_minus_fused_ms": round(ms["unfused"] - ms["fused"], 4), "grad_norm": norm, "coef_clip_on": coef_on}]

    # the passes alone, on the gradients the last step left
    c = idle.clipper
    a, b = idle.opt.begin, idle.opt.end                         # the optimizer's range: the segments and the padding between them
    grad = c.grad
    elems = sum(int(idle.model._ps.params[n].numel()) for n in c.names)
    state_on = c.state.clone()
    state_on[1] = 0.999
    state_idle = c.state.clone()
    state_idle[1] = 1.0
    fns = {"sqnorm": lambda: ops.grad_sqnorm(grad, c.table, c.partials, c.seg_norm, c.clip, c.state),
           "warm": lambda: ops.warm(grad[a:b]),
           "apply_on": lambda: ops.grad_clip_apply(grad, c.table, c.clip, state_on, "norm"),
           "apply_idle": lambda: ops.grad_clip_apply(grad, c.table, c.clip, state_idle, "norm")}
    for fn in fns.values():
        _events(fn, 3)
    u = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            u[k].append(_events(fn, calls) * 1e3)
    us = {k: round(med(v), 2) for k, v in u.items()}
    lines.append({"bench": "grad_clip_norm_pass", "segments": len(c.names), "workgroups": c.table[2], "elements": elems,
                  "bytes": elems * 4, "warm_bytes": (b - a) * 4, "calls": calls, "rounds": rounds, "us": us,
                  "spread": {k: round((max(v) - min(v)) / med(v), 3) for k, v in u.items()},
                  "sqnorm_over_warm": round(us["sqnorm"] / us["warm"], 3),
                  "sqnorm_GBps": round(elems * 4 / us["sqnorm"] / 1e3, 1), "warm_GBps": round((b - a) * 4 / us["warm"] / 1e3, 1)})
    for line in lines:
        s = json.dumps(line)
        print(s, flush=True)
        if out:
            with open(out, "a") as f:
                f.write(s + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20, help="training steps per measurement")
    ap.add_argument("--calls", type=int, default=20, help="kernel calls per measurement")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--out", metavar="FILE", help="append the JSON lines to FILE")
    a = ap.parse_args()
    run(a.batch, a.steps, a.calls, a.rounds, a.warmup, a.out)
