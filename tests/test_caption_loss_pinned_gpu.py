"""The three caption-loss entries (vct_sce_loss, vct_sce_loss_ls, vct_wce_loss) write today the bits they wrote before their kernels
were folded into one template (csrc/vct_caption_loss.hip).  tests/golden/caption_loss_parent_bits.json holds one sha256 per case of the
whole output arena (gpu_arena.Arena.buf: outputs, 0xFF fill and canaries), recorded by tools/make_golden_caption_loss_bits.py on an
MI355X in a checkout of the commit before the fold; this file recomputes each of them.  Cases and the call itself are the tool's
(cases(), run_case()): six rows of row_ref.sce_case, bf16 V in (9, 257, 32769) and fp32 V in (5, 257, 16385), in place / separate
dlogits with ld_dl = V rounded up + one vector / forward only, every alpha, smoothing and weight variant -- 144 calls.

The hashes pin that commit's bits UNDER THIS TOOLCHAIN (the fixture names it).  The fp64 tests (test_row_kernels_gpu.py,
test_label_smoothing_kernels_gpu.py, test_scst_gpu.py) say what is correct; this one says what is unchanged.  After a compiler change
the fixture is recorded again only once those tests pass."""
import importlib.util
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_golden_caption_loss_bits", os.path.join(ROOT, "tools", "make_golden_caption_loss_bits.py"))
T = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(T)

KINDS = ("sce", "ls", "wce")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from vct_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def pinned(golden_dir):
    with open(os.path.join(golden_dir, "caption_loss_parent_bits.json")) as f:
        return json.load(f)["sha256"]


def test_the_fixture_holds_exactly_the_cases(pinned):
    ids = [c[0] for c in T.cases()]
    assert len(ids) == len(set(ids)) == 144
    assert sorted(pinned) == sorted(ids)


@pytest.mark.parametrize("kind", KINDS)
def test_bits_of_the_commit_before_the_fold(ops, pinned, kind):
    changed = []
    for cid, *case in T.cases():
        if case[0] != kind:
            continue
        assert cid in pinned, f"{cid}: not in the fixture"
        a = T.run_case(ops, *case)
        if T.digest(a) != pinned[cid]:
            changed.append(cid)
        a.check(nonfinite_ok=("row_ws",) if kind == "wce" else ())     # (wce leaves the RCE rows of row_ws unwritten)
    assert not changed, f"{len(changed)} cases write other bits than the pinned commit: {changed}"
