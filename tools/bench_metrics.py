#!/usr/bin/env python
"""Caption-metric scoring benchmark, host against device, on a synthetic corpus at MSR-VTT's test-split scale: 2990 videos x 20
references of 5..14 words over a Zipf-like vocabulary, one 5..14-word candidate per video (plus end token and padding to 30
columns, as a decoder returns them).  Prints one JSON line per measurement and appends them to profiles/metrics_bench.jsonl:
  * table_build: metrics.CaptionMetrics(refs) (host tables), device_tables() and the upload, once per split;
  * host_score: CaptionMetrics.score over the 2990 candidates (plain Python, fp64), per evaluation;
  * device_score: DeviceCaptionMetrics.begin + add in batches of 128 + result (its one synchronisation), per evaluation, wall
    clock; device_only_ms is the same span between two stream events;
  * eval_metrics: evaluate.eval_metrics over a data.DeviceLoader of the same 2990 videos with the cfg-B model (bench.MODEL_CFG,
    untrained: it decodes to max_len), greedy, max_len 30, batch 128, at both levels, next to evaluate.eval_epoch (decoding to
    strings without scoring) over the same loader.
--videos / --refs shrink the corpus (a smoke run); --no-model skips the eval_metrics part."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

START, END, WORD0 = 101, 102, 1000
BATCH, MAX_LEN = 128, 30


def corpus(n_videos, n_refs, vocab=8000, seed=0):
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, vocab + 1)
    p /= p.sum()

    def sent():
        return (WORD0 + rng.choice(vocab, int(rng.integers(5, 15)), p=p)).tolist()
    refs = {f"video{v}": [sent() for _ in range(n_refs)] for v in range(n_videos)}
    # a candidate: one of the video's references with a third of its words redrawn (scores well away from 0 and 1)
    cands = {}
    for v, rs in refs.items():
        c = list(rs[int(rng.integers(len(rs)))])
        for j in range(len(c)):
            if rng.random() < 0.33:
                c[j] = WORD0 + int(rng.choice(vocab, p=p))
        cands[v] = c
    return refs, cands


def id_matrix(cands):
    ids = np.zeros((len(cands), MAX_LEN), np.int64)
    ids[:, 0] = START
    for i, c in enumerate(cands.values()):
        ids[i, 1:1 + len(c)] = c
        ids[i, 1 + len(c)] = END
    return ids


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return r, statistics.median(ts), min(ts)


class WordTok:
    """'w<id>' words <-> ids, standing in for the HF tokenizer (no vocabulary files offline)."""
    vocab_size = 30522
    _special = {"[PAD]": 0, "[CLS]": START, "[SEP]": END}

    def convert_tokens_to_ids(self, tok):
        return self._special[tok]

    def encode(self, text, **_):
        return [START] + [int(w[1:]) for w in text.split()] + [END]

    def convert_ids_to_tokens(self, ids):
        return [f"w{int(i)}" for i in ids]

    def convert_tokens_to_string(self, toks):
        return " ".join(toks)


def bench_scorers(refs, cands, out, reps):
    from vct_amd.metrics import CaptionMetrics
    dev = torch.device("cuda", 0)
    shape = {"videos": len(refs), "refs_per_video": len(next(iter(refs.values()))), "captions": len(cands)}
    t0 = time.perf_counter()
    cm = CaptionMetrics(refs, end_id=END)
    t1 = time.perf_counter()
    tables = cm.device_tables()
    t2 = time.perf_counter()
    from vct_amd.metrics import DeviceCaptionMetrics
    dm = DeviceCaptionMetrics(tables, dev)
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    emit({"bench": "table_build", **shape, "host_tables_ms": round((t1 - t0) * 1e3, 1), "device_tables_ms": round((t2 - t1) * 1e3, 1),
          "upload_ms": round((t3 - t2) * 1e3, 1), "ngrams": len(cm.cider.df), "ref_tokens": int(tables["ref_tok"].shape[0])}, out)

    host, host_ms, host_min = timed(lambda: cm.score(cands), max(1, reps // 4))
    ids = torch.from_numpy(id_matrix(cands)).to(dev)
    vids = list(cands)

    def device_eval():
        dm.begin(len(vids))
        for a in range(0, len(vids), BATCH):
            dm.add(ids[a:a + BATCH], vids[a:a + BATCH])
        return dm.result()
    device_eval()                                    # first call: module load, buffers
    got, dev_ms, dev_min = timed(device_eval, reps)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    spans = []
    for _ in range(reps):
        torch.cuda.synchronize()
        e0.record()
        device_eval()
        e1.record()
        e1.synchronize()
        spans.append(e0.elapsed_time(e1))
    worst = max(abs(got[k] - host[k]) / max(abs(host[k]), 1e-300) for k in host)
    emit({"bench": "host_score", **shape, "ms_per_eval": round(host_ms, 1), "min_ms": round(host_min, 1),
          "metrics": {k: round(v, 4) for k, v in host.items()}}, out)
    emit({"bench": "device_score", **shape, "batch": BATCH, "ms_per_eval": round(dev_ms, 3), "min_ms": round(dev_min, 3),
          "event_span_ms": round(statistics.median(spans), 3), "host_over_device": round(host_ms / dev_ms, 1),
          "worst_rel_diff_vs_host": float(f"{worst:.2e}"), "metrics": {k: round(v, 4) for k, v in got.items()}}, out)


def bench_eval_metrics(refs, out, reps):
    from bench import MODEL_CFG
    from vct_amd import data, evaluate
    from vct_amd.model import MMT4Caption
    dev = torch.device("cuda", 0)
    torch.manual_seed(666)
    m = MMT4Caption(MODEL_CFG, device=dev, compute_dtype=torch.bfloat16)
    m.mode("caption")
    m.eval()
    m.cap_preprocessor.tokenizer = WordTok()
    with tempfile.TemporaryDirectory() as d:
        os.makedirs(os.path.join(d, "feats"))
        rng = np.random.default_rng(1)
        with open(os.path.join(d, "split.txt"), "w") as f:
            for v, rs in refs.items():
                np.save(os.path.join(d, "feats", f"{v}.npy"), rng.standard_normal((12, 512)).astype(np.float32))
                for r in rs:
                    f.write(v + " " + " ".join(f"w{t}" for t in r) + "\n")
        ds = data.MSVD_Dataset([os.path.join(d, "feats")], os.path.join(d, "split.txt"), split_type="train", mode="by_video")
        dl = data.DeviceLoader(ds, BATCH, m.cap_preprocessor, dev, shuffle=False, feat_dtype=torch.bfloat16)
    shape = {"videos": len(ds), "refs_per_video": len(next(iter(refs.values()))), "batch": BATCH, "max_len": MAX_LEN, "dtype": "bf16"}

    def sync(fn):
        def run():
            r = fn()
            torch.cuda.synchronize()
            return r
        return run
    sync(lambda: evaluate.eval_epoch(m, dl, max_len=MAX_LEN))()             # graph capture, sessions
    _, dec_ms, _ = timed(sync(lambda: evaluate.eval_epoch(m, dl, max_len=MAX_LEN)), reps)
    emit({"bench": "eval_epoch_decode_only", **shape, "ms_per_eval": round(dec_ms, 1)}, out)
    for level in ("token", "word"):
        t0 = time.perf_counter()
        scorer = evaluate.build_scorer(m, ds.video2caption, level)
        build_ms = (time.perf_counter() - t0) * 1e3
        evaluate.eval_metrics(m, dl, max_len=MAX_LEN, level=level, scorer=scorer)
        res, ms, _ = timed(lambda: evaluate.eval_metrics(m, dl, max_len=MAX_LEN, level=level, scorer=scorer), reps)
        emit({"bench": "eval_metrics", "level": level, **shape, "scorer_build_ms": round(build_ms, 1), "ms_per_eval": round(ms, 1),
              "over_decode_only_ms": round(ms - dec_ms, 1), "sum": round(res["sum"], 6)}, out)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=2990)
    ap.add_argument("--refs", type=int, default=20)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--no-model", action="store_true", help="skip the eval_metrics-over-a-loader part")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metrics_bench.jsonl"))
    a = ap.parse_args()
    refs, cands = corpus(a.videos, a.refs)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as out:
        bench_scorers(refs, cands, out, a.reps)
        if not a.no_model:
            bench_eval_metrics(refs, out, a.reps)
