"""Cost of a second feature stream at cfg-B (d 512, 2 + 2 layers, V 30522, batch 256, captions of 20 tokens).

    python tools/bench_multimodal.py [--steps 30] [--warmup 8] [--rounds 3] [--out profiles/multimodal_bench.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o mm -- python tools/bench_multimodal.py --trace-only CASE
    python tools/bench_multimodal.py --summarize DIR --case CASE [--out FILE]     # front-end kernel times + bytes -> JSON

Cases in one process, measured in alternating rounds (a round runs every case once): one stream with T 12 (bench.py's headline
shape); two streams [512, 128] with T (12, 4) (S = 18) and T (12, 12) (S = 26); and the decoder-only A/B: the same model and batch
with the decoder's sample-stationary stack on and forced off (its _ss_ok gate), at one stream (S = 13) and at two streams with
T (12, 2) (S = 16, the largest memory the fused decoder takes).  Per case: ms/step and samples/s (CaptionTrainer, launch list,
FusedAdam: bench.py's executor), which stacks ran sample-stationary, and the greedy-decode token step at batch 128 (us/step,
captured step graphs replayed back to back, a fresh model).  --trace-only runs a few steps of one case for the profiler;
--summarize reduces that run's kernel_stats.csv to the two front-end kernels with the bytes they request."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

# (name, modal_shape, T per stream, decoder's sample-stationary stack allowed)
CASES = [("one_stream_T12", [512], (12,), True), ("two_streams_T12_4", [512, 128], (12, 4), True),
         ("two_streams_T12_12", [512, 128], (12, 12), True),
         ("one_stream_T12_dec_unfused", [512], (12,), False),
         ("two_streams_T12_2", [512, 128], (12, 2), True), ("two_streams_T12_2_dec_unfused", [512, 128], (12, 2), False)]


def model_for(shapes):
    import copy
    from vct_amd.model import MMT4Caption
    mc = copy.deepcopy(bench.MODEL_CFG)
    mc["modal"] = [f"m{i}" for i in range(len(shapes))]
    mc["modal_shape"] = list(shapes)
    torch.manual_seed(666)
    m = MMT4Caption(mc, device=torch.device("cuda"), compute_dtype=torch.bfloat16)
    m.mode("caption")
    return m


def batch_for(shapes, Ts, B):
    g = torch.Generator().manual_seed(0)
    feats = [torch.randn(B, t, e, generator=g).cuda() for e, t in zip(shapes, Ts)]
    masks = [torch.zeros(B, t, dtype=torch.bool).cuda() for t in Ts]
    ids = torch.randint(1000, 30000, (B, bench.S_TOK), generator=g)
    ids[:, 0], ids[:, -1] = 101, 102
    if len(shapes) == 1:
        return feats[0], masks[0], ids.cuda()
    return feats, masks, ids.cuda()


class Case:
    def __init__(self, name, shapes, Ts, B, dec_fused=True):
        from vct_amd import engine
        from vct_amd.trainer import CaptionTrainer, build_optimizer
        self.name, self.shapes, self.Ts, self.dec_fused = name, shapes, Ts, dec_fused
        self.model = model_for(shapes)
        self.model.train()
        if not dec_fused:           # this model's decoder only: its stack runs layer by layer whatever S is
            self.model.cap_decoder._engine().fuse_layers = False
        opt, _ = build_optimizer(bench.TRAIN_CFG, self.model)
        self.trainer = CaptionTrainer(self.model, opt, None, use_graph=False, launch_list=True)
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

    def decode_us(self, B=128):
        # a FRESH model (as bench.py's decode line): it practically never emits [SEP], so every caption runs all 29 steps
        m = model_for(self.shapes)
        m.eval()
        if not self.dec_fused:
            m.cap_decoder._engine().fuse_layers = False
        feats, masks, _ = batch_for(self.shapes, self.Ts, B)
        f = feats if isinstance(feats, list) else [feats]
        for _ in range(2):
            m.greedy_decode_ids(f, None, max_len=30)
        st = next((s for k, s in m.__dict__.get("_decode_sessions", {}).items() if k[0] == B), None)
        out = None
        if st is not None and all(t in st.graphs for t in range(1, 30)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(5):
                for t in range(1, 30):
                    st.graphs[t].replay()
            e1.record()
            torch.cuda.synchronize()
            out = round(e0.elapsed_time(e1) * 1e3 / (5 * 29), 1)
        return out


def frontend_bytes(kind, B, Ts, d=512, n_labels=None):
    """Bytes the front-end kernel requests (bf16 activations): forward = the unify outputs (2 B x rows) + the frame masks (1 B) read,
    the stack input and key-pad bytes written, + the fp32 temporal / modal tables; backward = d(stack input) read TWICE (once by the
    du workgroups, once by the modal-embedding reduction -- the second pass may hit in the cache) + du written + d_modal written."""
    S, T = sum(t + 1 for t in Ts), sum(Ts)
    n_labels = n_labels or 2 * len(Ts)
    if kind == "fwd":
        return 2 * B * T * d + B * T + 2 * B * S * d + B * S + 4 * (S + n_labels) * d
    return 2 * (2 * B * S * d) + 2 * B * T * d + 4 * n_labels * d


def summarize(trace_dir, case, batch, out):
    import csv
    import glob
    ts = dict((c[0], c[2]) for c in CASES)[case]
    paths = glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True)
    if not paths:
        raise SystemExit(f"no kernel_stats.csv under {trace_dir}")
    res = {"case": case, "batch": batch, "T": list(ts), "S": sum(t + 1 for t in ts), "kernels": {}}
    with open(paths[0]) as f:
        for r in csv.DictReader(f):
            name = r["Name"]
            for kind in ("fwd", "bwd"):
                if f"mm_frontend_{kind}_kernel" in name:
                    nbytes = frontend_bytes(kind, batch, ts)
                    avg, mn = float(r["AverageNs"]) / 1e3, float(r["MinNs"]) / 1e3
                    res["kernels"][kind] = {"calls": int(r["Calls"]), "avg_us": round(avg, 2), "min_us": round(mn, 2),
                                            "bytes_requested": nbytes, "GBps_at_min": round(nbytes / (mn * 1e-6) / 1e9, 1)}
    res["bytes_note"] = " ".join(frontend_bytes.__doc__.split(":", 1)[1].split())
    if out:
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--out", default=None, help="JSON result (default profiles/multimodal_bench.json; --summarize: stdout only)")
    ap.add_argument("--trace-only", metavar="CASE", help="a few steps of one case (for rocprofv3 --kernel-trace --stats)")
    ap.add_argument("--summarize", metavar="DIR", help="reduce the rocprofv3 --stats output of a --trace-only run")
    ap.add_argument("--case", help="--summarize: the case that run traced")
    args = ap.parse_args()
    if args.summarize:
        summarize(args.summarize, args.case, args.batch, args.out)
        return
    if args.trace_only:
        c = next(c for c in CASES if c[0] == args.trace_only)
        Case(c[0], c[1], c[2], args.batch, c[3]).run(5, 2)
        return
    cases = [Case(n, s, t, args.batch, f) for n, s, t, f in CASES]
    for _ in range(args.rounds):
        for c in cases:
            c.run(args.steps, args.warmup)
    res = {"batch": args.batch, "steps": args.steps, "rounds": args.rounds, "cases": {}}
    for c in cases:
        ms = sorted(c.times)[len(c.times) // 2]
        res["cases"][c.name] = {"modal_shape": c.shapes, "T": list(c.Ts), "S": sum(t + 1 for t in c.Ts),
                                "decoder_fused_allowed": c.dec_fused,
                                "ms_per_step_median": round(ms, 4), "ms_per_step_rounds": [round(t, 4) for t in c.times],
                                "samples_per_s": round(args.batch / ms * 1e3, 1), "sample_stationary_stacks": c.ss,
                                "decode_b128_us_per_step": c.decode_us()}
    out = args.out or os.path.join(ROOT, "profiles", "multimodal_bench.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
