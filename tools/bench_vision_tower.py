"""Cost of the CLIP vision tower (vct_amd.vision.ClipVisionTower) at the ViT-B/32 shape -- 12 layers x width 768, 12 heads, ff 3072,
32 x 32 patches of a 224 px image (50 rows per frame), projection 512, random weights, bf16 -- on uint8 frames of 360 x 640.

    python tools/bench_vision_tower.py [--frames 2048] [--chunk 256] [--out profiles/vision_tower_bench.jsonl]

Two loads, each as the median of 9 timings between stream events after a warm-up call:
  video     one video's 20 frames, from host memory: encode_frames (the copy to the device included)
  frames    2 048 frames from host memory through encode_all in chunks
and next to them, alternating with ours inside the same rounds, the path this replaces: PIL on the host (resize, crop, the same value
table) and transformers' CLIPVisionModelWithProjection in bf16 on the same GPU.  Where PIL or transformers do not import the torch side
is left out and the record says so.  One more record: vct_frames_to_patches alone on device-resident frames against the bytes it has
to move (the frames in, the patch matrix out).  Outputs of both sides are compared (relative Frobenius) with each other and, on two
frames, with the fp64 restatement, so a fast wrong answer cannot pass as a time."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPE = dict(W=768, H=12, ff=3072, layers=12, P_out=512, patch=32, R=224)
FRAME = (360, 640)


def torch_side(sd):
    """(name, callable uint8 host frames [N, H, W, 3] -> fp32 [N, P_out] on the device) or (reason, None)."""
    try:
        import vision_ref as R
        from PIL import Image
        from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
    except ImportError as e:
        return f"left out: {e}", None
    cfg = CLIPVisionConfig(hidden_size=SHAPE["W"], intermediate_size=SHAPE["ff"], num_hidden_layers=SHAPE["layers"],
                           num_attention_heads=SHAPE["H"], image_size=SHAPE["R"], patch_size=SHAPE["patch"],
                           projection_dim=SHAPE["P_out"], hidden_act="quick_gelu")
    m = CLIPVisionModelWithProjection(cfg)
    m.load_state_dict(R.openai_to_transformers(sd), strict=False)
    m = m.to(torch.bfloat16).cuda().eval()
    lut = R.value_table(dtype=torch.bfloat16)
    Rr = SHAPE["R"]

    @torch.no_grad()
    def run(frames, chunk=256):
        outs = []
        for i in range(0, frames.shape[0], chunk):
            crops = []
            for f in frames[i:i + chunk].numpy():
                oh, ow = R.resized_size(f.shape[0], f.shape[1], Rr)
                top, left = R.crop_offsets(oh, ow, Rr)
                crops.append(np.asarray(Image.fromarray(f).resize((ow, oh), Image.BICUBIC).crop((left, top, left + Rr, top + Rr))))
            crop = torch.from_numpy(np.stack(crops))
            pixels = torch.stack([lut[c][crop[..., c].long()] for c in range(3)], 1)
            outs.append(m(pixel_values=pixels.cuda(non_blocking=True)).image_embeds.float())
        return torch.cat(outs)
    return "PIL on the host + transformers.CLIPVisionModelWithProjection bf16", run


def median9(fns, warm=1):
    """The callables timed in turn inside each of 9 rounds (neighbours in time), each between stream events -> [(median, all)]."""
    for _ in range(warm):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(9):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts[k].append(e0.elapsed_time(e1))
    return [(sorted(t)[4], t) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=2048)
    ap.add_argument("--chunk", type=int, default=256)
    ap.add_argument("--video", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_vision_tower.py measures on the GPU; there is none here")
    import vision_ref as R
    from vct_amd import ops
    from vct_amd.vision import ClipVisionTower
    sd = R.random_state_dict(SHAPE["W"], SHAPE["ff"], SHAPE["layers"], SHAPE["P_out"], SHAPE["patch"], SHAPE["R"], seed=1, std=0.03)
    tower = ClipVisionTower.from_state_dict(sd, "cuda", torch.bfloat16)
    tname, ttower = torch_side(sd)
    H, W = FRAME
    video = torch.from_numpy(R.random_frames(args.video, H, W, seed=2))
    frames = torch.from_numpy(R.random_frames(args.frames, H, W, seed=3)).pin_memory()
    out_all = torch.empty(args.frames, SHAPE["P_out"], device="cuda")
    rel = lambda x, y: float((x.double() - y.double()).norm() / y.double().norm())      # noqa: E731
    recs = []
    loads = (("video", video, lambda: tower.encode_frames(video)), ("frames", frames, lambda: tower.encode_all(frames, args.chunk, out_all)))
    for name, data, f_ours in loads:
        fns = [f_ours] + ([lambda d=data: ttower(d, args.chunk)] if ttower else [])
        res = median9(fns)
        n = data.shape[0]
        rec = {"record": name, "frames": n, "frame_size": list(FRAME), "chunk": args.chunk if name == "frames" else None, "shape": SHAPE,
               "compute_dtype": "bf16", "input": "host memory, copy included", "ours_ms_median9": round(res[0][0], 4),
               "ours_ms_all": [round(t, 4) for t in res[0][1]], "frames_per_s_ours": round(n / res[0][0] * 1e3, 1),
               "launches_per_call_ours": (7 * SHAPE["layers"] + 5) * (1 if name == "video" else -(-n // args.chunk)), "torch_side": tname}
        if ttower:
            rec.update(torch_ms_median9=round(res[1][0], 4), torch_ms_all=[round(t, 4) for t in res[1][1]],
                       ours_over_torch=round(res[0][0] / res[1][0], 4), frames_per_s_torch=round(n / res[1][0] * 1e3, 1))
        recs.append(rec)
    a = tower.encode_frames(video)
    exact = R.tower(sd, video[:2], SHAPE["H"]).cuda()
    agree = {"record": "agreement_video", "rel_frobenius_ours_vs_fp64_first2": round(rel(a[:2], exact), 6)}
    if ttower:
        b = ttower(video)
        agree.update(rel_frobenius_ours_vs_torch=round(rel(a, b), 6), rel_frobenius_torch_vs_fp64_first2=round(rel(b[:2], exact), 6))
    recs.append(agree)
    # the preprocessing kernel alone, on device-resident frames, one launch per chunk
    P, Rr = SHAPE["patch"], SHAPE["R"]
    G = Rr // P
    dev_frames = frames[:args.chunk].cuda()
    n = dev_frames.shape[0]
    a_op = torch.empty(n * G * G, 3 * P * P, dtype=torch.bfloat16, device="cuda")
    tables = tower.tables(H, W)
    (ms, all_ms), = median9([lambda: ops.frames_to_patches(dev_frames, tables, tower.lut, P, a_op)], warm=2)
    moved = dev_frames.numel() + a_op.numel() * 2
    recs.append({"record": "frames_to_patches_alone", "frames": n, "frame_size": list(FRAME), "ms_median9": round(ms, 4),
                 "ms_all": [round(t, 4) for t in all_ms], "bytes_in": dev_frames.numel(), "bytes_out": a_op.numel() * 2,
                 "gb_per_s": round(moved / ms * 1e-6, 1), "staged_rows_per_patch": int(tables["stage_rows"][P]),
                 "note": "bytes_in counts whole frames; the centre crop (224 of 398 resized columns) leaves about 44 % of each row unread"})
    out = args.out or os.path.join(ROOT, "profiles", "vision_tower_bench.jsonl")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        for r in recs:
            f.write(json.dumps(r) + "\n")
            print(json.dumps(r))


if __name__ == "__main__":
    main()
