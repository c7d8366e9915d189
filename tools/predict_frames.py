"""Caption a clip given as frames: the counterpart of the reference's `predict_video.py --video`, on the device from the uint8 frames
to the token ids (vct_amd.vision.ClipVisionTower -> evaluate.v2t_frames).

    python tools/predict_frames.py --config CONFIG.json --model MODEL.pth --clip-weights CLIP.pt --frames DIR|FILE.npy [--beam K]

--frames: a directory of images (read with PIL in name order, converted to RGB; all of one size) or an .npy of uint8 [T, H, W, 3] RGB
frames.  Decoding the video and choosing which frames to keep are the caller's: no decoder and no sampling policy are shipped.
--clip-weights: a CLIP state dict in OpenAI's or transformers' key convention (ViT-B/32; --clip-prefix clip. for a CLIP4Clip
checkpoint); no weights are shipped either.  --greedy is the default; --beam K searches K beams.  Generation controls (both
decoders; vct_amd.decode.GenerationControls): --min-length N (no end token before N tokens), --no-repeat-ngram N (no n-gram twice),
--repetition-penalty THETA (>= 1), --ban ID [ID ...] (token ids that are never emitted).  Prints `id<TAB>caption`."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def read_frames(path: str) -> torch.Tensor:
    """-> uint8 [T, H, W, 3] on the host."""
    if os.path.isdir(path):
        from PIL import Image
        names = sorted(n for n in os.listdir(path) if n.lower().endswith((".jpg", ".jpeg", ".png", ".bmp", ".webp")))
        if not names:
            raise SystemExit(f"{path} holds no image")
        frames = [np.asarray(Image.open(os.path.join(path, n)).convert("RGB")) for n in names]
        if len({f.shape for f in frames}) != 1:
            raise SystemExit(f"the images in {path} differ in size; one clip's frames share a size")
        arr = np.stack(frames)
    else:
        arr = np.load(path, allow_pickle=False)
    if arr.dtype != np.uint8 or arr.ndim != 4 or arr.shape[3] != 3 or arr.shape[0] < 1:
        raise SystemExit(f"{path}: expected uint8 [T, H, W, 3] RGB frames, got {arr.dtype} {arr.shape}")
    return torch.from_numpy(np.ascontiguousarray(arr))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", required=True)
    ap.add_argument("--model", required=True)
    ap.add_argument("--clip-weights", required=True)
    ap.add_argument("--clip-prefix", default="")
    ap.add_argument("--frames", required=True, nargs="+", help="one or more directories / .npy files, one caption each")
    mode = ap.add_mutually_exclusive_group()
    mode.add_argument("--greedy", action="store_true")
    mode.add_argument("--beam", type=int, default=None, metavar="K")
    ap.add_argument("--max-len", type=int, default=30)
    ap.add_argument("--fp32", action="store_true", help="parity mode: fp32 GEMM operands in the tower and the model")
    ap.add_argument("--min-length", type=int, default=0, metavar="N", help="at least N tokens before the end token")
    ap.add_argument("--no-repeat-ngram", type=int, default=0, metavar="N", help="no n-gram of this size twice in a caption (0 = off, at most 8)")
    ap.add_argument("--repetition-penalty", type=float, default=1.0, metavar="THETA", help="1 = off, at most 16")
    ap.add_argument("--ban", type=int, nargs="+", default=[], metavar="ID", help="token ids that are never emitted (at most 32)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("predict_frames.py runs on the GPU; there is none here")
    from vct_amd import checkpoint, evaluate
    from vct_amd.decode import GenerationControls
    try:
        controls = GenerationControls(args.min_length, args.no_repeat_ngram, args.repetition_penalty, args.ban)
    except ValueError as e:
        raise SystemExit(str(e))
    from vct_amd.model import MMT4Caption
    from vct_amd.utils import Config
    from vct_amd.vision import ClipVisionTower
    cfg = Config(args.config)
    cfg.check()
    dev = torch.device("cuda", 0)
    dtype = torch.float32 if args.fp32 else torch.bfloat16
    model = MMT4Caption(cfg.data["model"], device=dev, compute_dtype=dtype)
    model.mode("caption")
    checkpoint.load_weights(model, args.model)
    tower = ClipVisionTower.from_file(args.clip_weights, dev, dtype, prefix=args.clip_prefix)
    videos = [read_frames(p) for p in args.frames]
    captions = evaluate.v2t_frames(model, tower, videos, max_len=args.max_len, beam_size=args.beam, controls=controls)
    for p, c in zip(args.frames, captions):
        print(f"{os.path.splitext(os.path.basename(os.path.normpath(p)))[0]}\t{c}")


if __name__ == "__main__":
    main()
