"""Pick tests/ensemble_ref.py's GAP_SEED: the first batch seed for which, along the ensemble's own greedy ids, the fp64 reference's
top-2 gap exceeds the reference's bound at every position of every row, for both batch sizes and both modes of
tests/test_ensemble_gpu.py::test_every_greedy_token_is_the_fp64_argmax (which asserts that condition before it looks at a token).

    python tools/pick_ensemble_seed.py [first_seed [how_many]]     # needs a GPU

Prints one line per seed with the smallest gap / bound ratio seen, then the seed to record."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import ensemble_ref as ER  # noqa: E402
from vct_amd import decode  # noqa: E402

DEV, MAX_LEN, W = "cuda", 10, [0.6, 0.4]


def worst_ratio(a, b, seed):
    worst = float("inf")
    for B in (1, 3):
        feats = ER.tiny_batch(B, seed, DEV)
        for mode in ("prob", "logprob"):
            ys = decode.Ensemble([a, b], weights=W, mode=mode).greedy_decode_ids(feats, None, MAX_LEN)
            steps = ys.shape[1] - 1
            logits = [decode.teacher_forced_next_ids(m, feats, None, ys, steps, return_logits=True)[1].reshape(-1, ER.V_TINY) for m in (a, b)]
            out, bound = ER.combine(logits, W, decode.ensemble.MODES[mode])
            top = out.topk(2, dim=1)
            ratio = (top.values[:, 0] - top.values[:, 1]) / bound.gather(1, top.indices).sum(1)
            worst = min(worst, float(ratio.min()))
    return worst


def main():
    first = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    count = int(sys.argv[2]) if len(sys.argv) > 2 else 16
    a, b = ER.tiny_models(DEV)
    picked = None
    for seed in range(first, first + count):
        r = worst_ratio(a, b, seed)
        print(f"seed {seed}: smallest top-2 gap / bound = {r:.2f}")
        if picked is None and r > 1.0:
            picked = seed
    print(f"GAP_SEED = {picked}")


if __name__ == "__main__":
    with torch.no_grad():
        main()
