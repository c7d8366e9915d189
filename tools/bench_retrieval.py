#!/usr/bin/env python
"""Text-video retrieval scoring benchmark on synthetic embeddings: 1 000 texts x 1 000 videos and MSR-VTT's test split, 59 800
texts x 2 990 videos (20 captions per video), at Dt = 512, in both modes (plain; dual softmax with tau = 0.05).  v is standard
normal, t = v[gt] + 6 * noise (about where rank 1 is lost at this Dt, so that the ranks are spread).  Prints one JSON line per case
and appends it to profiles/retrieval_bench.jsonl:
  * device_ms: ops.retrieval_ranks (csrc/vct_retrieval.hip: the matrix is never stored), all launches between two stream events;
    phase_ms: the same for each phase alone (prep = norms and zeroing, stats = the column-statistics sweep of the dual softmax,
    gt = ground-truth scores and best own text, count = the counting sweep, finish = ranks -> statistics);
  * torch_ms: the straightforward materialising fp32 version on the same GPU (normalise, matmul, softmax over dim 0, gather,
    comparisons, sums, sort for the median) -- the yardstick for the device scorer;
  * host_ms: retrieval.RetrievalMetrics (numpy fp64 on the materialised matrix), wall clock, one run at the large shape.
Every timing is the median of --reps runs after --warmup runs (the host scorer apart).  The record also carries each scorer's
rsum and how many ranks differ between the device and torch versions (both fp32, different summation orders: near-ties may
differ), so that a case that measured nothing, or two cases that measured the same thing, show."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DT, TAU = 512, 0.05
CASES = [(1000, 1), (2990, 20)]                # (videos, captions per video)
PHASES = ("prep", "stats", "gt", "count", "finish")


def embeddings(n_videos, per, seed=0):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((n_videos, DT)).astype(np.float32)
    gt = np.repeat(np.arange(n_videos), per).astype(np.int32)
    t = v[gt] + 6.0 * rng.standard_normal((gt.size, DT)).astype(np.float32)
    return t, v, gt


def torch_ranks(t, v, gt, mode, tau):
    """The materialising version: (ranks_t2v, ranks_v2t, stats [12]) as device tensors."""
    s = torch.nn.functional.normalize(t, dim=1) @ torch.nn.functional.normalize(v, dim=1).T
    f = s if mode == "plain" else s * torch.softmax(s / tau, dim=0)
    Nt, Nv = f.shape
    g = gt.long()
    jj, ii = torch.arange(Nv, device=f.device), torch.arange(Nt, device=f.device)
    fg = f.gather(1, g[:, None])
    rt = 1 + ((f > fg) | ((f == fg) & (jj[None, :] < g[:, None]))).sum(1)
    own = g[:, None] == jj[None, :]
    fo = torch.where(own, f, torch.full_like(f, float("-inf")))
    fb = fo.max(0).values
    ib = torch.where(own & (fo == fb[None, :]), ii[:, None], Nt).min(0).values
    rv = 1 + ((f > fb[None, :]) | ((f == fb[None, :]) & (ii[:, None] < ib[None, :]))).sum(0)
    rv = torch.where(ib < Nt, rv, torch.zeros_like(rv))
    out = []
    for r in (rt, rv):
        q = r[r > 0].double()
        srt = q.sort().values
        n = srt.numel()
        out += [(q <= 1).double().mean(), (q <= 5).double().mean(), (q <= 10).double().mean(),
                0.5 * (srt[(n - 1) // 2] + srt[n // 2]), q.mean(), torch.tensor(float(n), dtype=torch.float64, device=f.device)]
    return rt, rv, torch.stack(out)


def span_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), min(ts)


def rsum(stats12):
    return 100.0 * float(sum(stats12[k] for k in (0, 1, 2, 6, 7, 8)))


def run_case(n_videos, per, mode, out, reps, warmup, host):
    from vct_amd import ops
    from vct_amd.retrieval import RetrievalMetrics
    dev = torch.device("cuda", 0)
    t, v, gt = embeddings(n_videos, per)
    dt, dv, dg = (torch.from_numpy(a).to(dev) for a in (t, v, gt))
    tau = TAU if mode == "dual_softmax" else None
    dtau = torch.tensor([tau], dtype=torch.float32, device=dev) if tau is not None else None
    Nt, Nv = gt.size, n_videos
    rt = torch.empty(Nt, dtype=torch.int32, device=dev)
    rv = torch.empty(Nv, dtype=torch.int32, device=dev)
    o = torch.empty(12, dtype=torch.float64, device=dev)
    ws = torch.empty(ops.retrieval_workspace_bytes(Nt, Nv, DT, mode), dtype=torch.uint8, device=dev)

    def device(phases=None):
        return ops.retrieval_ranks(dt, dv, dg, rt, rv, o, ws, mode=mode, tau=dtau, phases=phases)
    dev_ms, dev_min = span_ms(device, reps, warmup)
    phase_ms = {}
    for ph in PHASES:                           # (the full runs above left the workspace every phase reads)
        if ph == "stats" and mode == "plain":
            continue
        phase_ms[ph] = round(span_ms(lambda: device((ph,)), reps, 1)[0], 4)
    device()
    d_stats = o.tolist()
    tor_ms, tor_min = span_ms(lambda: torch_ranks(dt, dv, dg, mode, tau), reps, warmup)
    trt, trv, tstats = torch_ranks(dt, dv, dg, mode, tau)
    differ = int((trt.int() != rt).sum()) + int((trv.int() != rv).sum())
    rec = {"bench": "retrieval", "texts": Nt, "videos": Nv, "Dt": DT, "mode": mode, "tau": tau, "reps": reps, "warmup": warmup,
           "device_ms": round(dev_ms, 4), "device_min_ms": round(dev_min, 4), "phase_ms": phase_ms,
           "torch_ms": round(tor_ms, 4), "torch_min_ms": round(tor_min, 4), "torch_over_device": round(tor_ms / dev_ms, 3),
           "workspace_mb": round(ws.numel() / 2 ** 20, 2), "matrix_mb_never_stored": round(Nt * Nv * 4 / 2 ** 20, 1),
           "device_rsum": round(rsum(d_stats), 4), "torch_rsum": round(rsum(tstats.tolist()), 4), "ranks_differing_device_vs_torch": differ,
           "device_median_mean": [d_stats[3], round(d_stats[4], 4), d_stats[9], round(d_stats[10], 4)]}
    if host:
        h = RetrievalMetrics(mode, tau)
        t0 = time.perf_counter()
        hs = h.score(t, v, gt)
        rec["host_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        rec["host_rsum"] = round(hs["rsum"], 4)
        rec["host_over_device"] = round(rec["host_ms"] / dev_ms, 1)
    line = json.dumps(rec)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()
    return rec


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-host", action="store_true", help="skip the numpy fp64 host scorer (slow at the large shape)")
    ap.add_argument("--small", action="store_true", help="only the 1 000 x 1 000 case (a smoke run)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "retrieval_bench.jsonl"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    recs = []
    with open(a.out, "a") as out:
        for n_videos, per in (CASES[:1] if a.small else CASES):
            for mode in ("plain", "dual_softmax"):
                recs.append(run_case(n_videos, per, mode, out, a.reps, a.warmup, not a.no_host))
    # cases that measured the same thing would show as equal outputs
    assert len({(r["device_rsum"], r["texts"]) for r in recs}) == len(recs), "two cases produced the same result"
