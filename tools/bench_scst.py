#!/usr/bin/env python
"""Self-critical training benchmark: the benchmark model (bench.MODEL_CFG, bf16, train mode) on synthetic (videos, 12, 512)
features, N = 5 sampled captions per video, max_len 30, CIDEr-D over 5 synthetic references per video.  The three stages of
CaptionTrainer.scst_step are timed separately, median over the rounds, one JSON line:
  * sample_ms: model.sample_decode_ids (videos x N rows on the KV-cached decode step), wall time around a device sync;
  * reward_ms: rewards.CiderD on the host (ids already on the host) + the leave-one-out advantages;
  * train_ms:  model.train_step_kernels_scst + the optimizer step (device time, HIP events);
  * step_ms:   CaptionTrainer.scst_step end to end (wall time, includes the device -> host copy of the ids);
  * caption_step_ms: CaptionTrainer.step (eager executor) on videos x N captions of the same length, for scale.
--device-reward adds, in the same process and on the same sampled ids:
  * reward_dev_ms: the device stage (ops.cider_d behind rewards.CiderD.to_device() + ops.scst_advantages), HIP events;
  * step_dev_ms:   CaptionTrainer.scst_step end to end with the device reward (wall time);
  * tables_ms:     the one-time build and upload of the reference tables (CiderD.to_device), wall time;
  * reward_max_diff: the largest |device - host| reward of the last round (the parity test is tests/test_cider_device_gpu.py).
--out FILE appends the line to FILE (profiles/scst_bench.jsonl)."""
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
from bench import MODEL_CFG  # noqa: E402

MAX_LEN = 30


def _refs(videos, vocab, seed=0, per_video=5):
    rng = np.random.default_rng(seed)
    return {v: [[int(t) for t in rng.integers(1000, min(30000, vocab), int(rng.integers(6, 20)))] + [102] for _ in range(per_video)]
            for v in range(videos)}


def _wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def run(videos: int, samples: int, rounds: int, out=None, device_reward: bool = False):
    from vct_amd import ops
    from vct_amd.model import MMT4Caption
    from vct_amd.rewards import CiderD, advantages
    from vct_amd.trainer import CaptionTrainer, FusedAdam
    dev = torch.device("cuda", 0)
    torch.manual_seed(666)
    m = MMT4Caption(MODEL_CFG, device=dev, compute_dtype=torch.bfloat16)
    m.mode("caption")
    m.train()
    tr = CaptionTrainer(m, FusedAdam(m, lr=1e-4))
    V = m.cap_preprocessor.tokenizer.vocab_size
    feats = torch.randn(videos, 12, 512, generator=torch.Generator().manual_seed(0)).to(dev)
    mask = torch.zeros(videos, 12, dtype=torch.bool, device=dev)
    reward_fn = CiderD(_refs(videos, V))
    vids = list(range(videos))
    kw = dict(num_samples=samples, max_len=MAX_LEN)
    for s in range(2):                                    # warm-up: sessions captured, buffers grown
        tr.scst_step(feats, mask, reward_fn, vids, seed=s, **kw)
    dev_fn, extra = None, {}
    if device_reward:
        t0 = time.perf_counter()
        dev_fn = reward_fn.to_device(dev)
        torch.cuda.synchronize()
        extra["tables_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        for s in range(2):
            tr.scst_step(feats, mask, dev_fn, vids, seed=s, **kw)
    t_sample, t_reward, t_train, t_step, t_cap, t_reward_dev, t_step_dev = [], [], [], [], [], [], []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ids = None
    for r in range(rounds):
        ms, ids = _wall(lambda: m.sample_decode_ids(feats, mask, seed=100 + r, **kw))
        t_sample.append(ms)
        host = ids.cpu()
        t0 = time.perf_counter()
        adv = advantages(reward_fn(host, vids), "mean_others")
        t_reward.append((time.perf_counter() - t0) * 1e3)
        if dev_fn is not None:
            torch.cuda.synchronize()
            e0.record()
            r_dev = dev_fn(ids, vids)
            adv_dev = ops.scst_advantages(r_dev)[0]
            e1.record()
            e1.synchronize()
            t_reward_dev.append(e0.elapsed_time(e1))
            extra["reward_max_diff"] = float((r_dev.cpu() - torch.from_numpy(reward_fn(host, vids))).abs().max())
            extra["adv_max_diff"] = float((adv_dev.cpu() - torch.from_numpy(adv.reshape(-1))).abs().max())
        seq_w = torch.from_numpy(adv.reshape(-1).copy()).to(dev)
        flat = ids.view(videos * samples, -1)
        torch.cuda.synchronize()
        e0.record()
        m.train_step_kernels_scst(feats, mask, flat, seq_w, samples)
        tr.opt.step()
        e1.record()
        e1.synchronize()
        t_train.append(e0.elapsed_time(e1))
        t_step.append(_wall(lambda: tr.scst_step(feats, mask, reward_fn, vids, seed=200 + r, **kw))[0])
        if dev_fn is not None:
            t_step_dev.append(_wall(lambda: tr.scst_step(feats, mask, dev_fn, vids, seed=200 + r, **kw))[0])
    # for scale: the caption step on as many rows of the same length (eager executor, the fusion this step keeps off is on there)
    f2, k2 = feats.repeat_interleave(samples, 0), mask.repeat_interleave(samples, 0)
    cap_ids = ids.view(videos * samples, -1).clone()
    for _ in range(2):
        tr.step(f2, k2, cap_ids)
    for r in range(rounds):
        t_cap.append(_wall(lambda: tr.step(f2, k2, cap_ids))[0])
    med = statistics.median
    if dev_fn is not None:
        extra.update(reward_dev_ms=round(med(t_reward_dev), 3), step_dev_ms=round(med(t_step_dev), 3))
    line = json.dumps({"bench": "scst", "dtype": "bfloat16", "videos": videos, "samples": samples, "rows": videos * samples,
                       "max_len": MAX_LEN, "sampled_len": int(ids.shape[2]), "rounds": rounds,
                       "sample_ms": round(med(t_sample), 3), "reward_ms": round(med(t_reward), 3), "train_ms": round(med(t_train), 3),
                       "step_ms": round(med(t_step), 3), "caption_step_ms": round(med(t_cap), 3),
                       "train_spread": round((max(t_train) - min(t_train)) / med(t_train), 3), **extra})
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=256, help="videos per step (the benchmark's per-GPU batch)")
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", metavar="FILE", help="append the JSON line to FILE")
    ap.add_argument("--device-reward", action="store_true", help="also time the reward on the device (CiderD.to_device)")
    a = ap.parse_args()
    run(a.videos, a.samples, a.rounds, a.out, a.device_reward)
