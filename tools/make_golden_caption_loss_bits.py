#!/usr/bin/env python
"""Record tests/golden/caption_loss_parent_bits.json: one sha256 per case of everything the three caption-loss entries (vct_sce_loss,
vct_sce_loss_ls, vct_wce_loss) write, taken over the whole output arena of the call (tests/gpu_arena.py Arena.buf: the outputs, the
0xFF fill around and between them, the canaries).  A changed bit, a word that used to be left untouched and a write outside the
outputs all change the hash.

    python tools/make_golden_caption_loss_bits.py [--commit TEXT]        # needs an MI355X; run in a checkout of the commit to pin

Uses vct_amd.ops, tests/row_ref.py and tests/gpu_arena.py only.  tests/test_caption_loss_pinned_gpu.py imports cases() and run_case()
from here and recomputes every hash.

Cases (144 calls of six rows): rows of row_ref.sce_case (B 3, S 2: dominant label, label below the RCE clamp, random row, pad tail,
all-pad sequence), logits with NaN in the columns V..ldl-1 and in the row behind N;
    bf16 V in (9, 257, 32769), fp32 V in (5, 257, 16385): a vector tail, the small instantiation, the first width of the large one;
    forms   inplace; separate (dlogits with ld_dl = V rounded up + one vector); forward (no dlogits);
    sce     alpha in (1.0, 0.5);
    ls      alpha in (1.0, 0.5) x smoothing in (0.0, 0.1), with the statistics;
    wce     seq_w None or a seeded random fp32 [B], with tok_logp."""
import argparse
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import row_ref as R  # noqa: E402
from gpu_arena import Arena, up  # noqa: E402

DEV = "cuda"
F32, BF = R.F32, R.BF
FIXTURE = os.path.join(ROOT, "tests", "golden", "caption_loss_parent_bits.json")
SHAPES_V = {BF: (9, 257, 32769), F32: (5, 257, 16385)}
FORMS = ("inplace", "separate", "forward")
VARIANTS = ([("sce", dict(alpha=a)) for a in (1.0, 0.5)]
            + [("ls", dict(alpha=a, eps=e)) for a in (1.0, 0.5) for e in (0.0, 0.1)]
            + [("wce", dict(weights=w)) for w in (False, True)])
SEED_ROWS, SEED_W = 40, 41


def cases():
    """[(id, kind, dtype, V, form, parameters)] in a fixed order."""
    out = []
    for dtype, name in ((BF, "bf16"), (F32, "fp32")):
        for V in SHAPES_V[dtype]:
            for kind, par in VARIANTS:
                for form in FORMS:
                    tag = "-".join(f"{k}={v}" for k, v in par.items())
                    out.append((f"{kind}-{name}-V{V}-{tag}-{form}", kind, dtype, V, form, par))
    return out


def run_case(ops, kind, dtype, V, form, par):
    """One call on a fresh arena; returns the arena (not synchronised)."""
    x, ids, pad = R.sce_case(V, SEED_ROWS, dtype)
    x, ids = x.to(DEV), ids.to(DEV)
    v = R.vec_of(dtype)
    N, vr = x.shape[0], up(V, v)
    labels = ids[:, 1:]
    nws = 4 * N + 1 if kind == "ls" else 2 * N + 1
    specs = [("loss", 1, 1, F32, 1, 0), ("row_ws", 1, nws, F32, nws + 1, 0)]
    if kind == "ls":
        specs.append(("stats", 1, 2, F32, 2, 0))
    if kind == "wce":
        specs.append(("tok_logp", 1, N, F32, N, 0))
    if form == "inplace":
        a = Arena(specs + [("dl", N, vr, dtype, vr, 0)])
        a["dl"][:, :V] = x
        logits = dl = a["dl"]
    else:
        buf = torch.full((N + 1, vr + v), float("nan"), dtype=dtype, device=DEV)
        buf[:N, :V] = x
        logits, dl = buf[:N], None
        a = Arena(specs + ([("dl", N, vr + v, dtype, vr + v, 0)] if form == "separate" else []))
        if form == "separate":
            dl = a["dl"]
    S = labels.shape[1]
    if kind == "sce":
        ops.sce_loss(logits, V, labels, S, pad, par["alpha"], a["loss"], dl, a["row_ws"])
    elif kind == "ls":
        ops.sce_loss_ls(logits, V, labels, S, pad, par["alpha"], par["eps"], a["loss"], dl, a["row_ws"], stats=a["stats"].view(-1))
    else:
        w = None
        if par["weights"]:
            w = (0.25 + torch.rand(N // S, generator=torch.Generator().manual_seed(SEED_W))).to(DEV)
        ops.wce_loss(logits, V, labels, S, pad, w, a["loss"], dl, a["row_ws"], tok_logp=a["tok_logp"].view(-1))
    return a


def digest(arena):
    torch.cuda.synchronize()
    return hashlib.sha256(arena.buf.cpu().numpy().tobytes()).hexdigest()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default="", help="copied into the fixture: the commit whose bits these are")
    ap.add_argument("--out", default=FIXTURE)
    a = ap.parse_args()
    from vct_amd import ops
    sha = {}
    for cid, *case in cases():
        sha[cid] = digest(run_case(ops, *case))
        assert sha[cid] == digest(run_case(ops, *case)), f"{cid}: two calls differ"
    with open(a.out, "w") as f:
        json.dump({"commit": a.commit, "device": torch.cuda.get_device_name(0), "hip": torch.version.hip, "sha256": sha}, f, indent=1)
        f.write("\n")
    print(f"{len(sha)} cases -> {a.out}")
