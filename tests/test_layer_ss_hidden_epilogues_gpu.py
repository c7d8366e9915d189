"""The fused stack forward with the last feed-forward chunk's GELU / dropout epilogue issued from the linear2 slice in front of it, and
the LayerNorm epilogues' dropout masks hashed as keep bits between the K steps of the product in front of each norm
(csrc/vct_layer_ss.hip: the chunk loop; csrc/vct_layer_ss_core.h: ln_keep_slice, epi_ln).

What can go wrong, and where it shows:
  * the moved epilogue writes the activation buffer HP[(nj - 1) & 1] while another wave still reads it (linear2(nj - 3), the copy it
    carried, or at nj = 2 the a2 / v copy that linear1(0) / out_proj carried): h, f, n3.* differ from the reference or between two launches;
  * a keep bit at the wrong position, of the wrong element or of the wrong site: every tensor behind that dropout (n1.y / n2.y / n3.y and
    what follows) differs from the fp64 reference, whose mask is the counter hash of (seed, site, element index), and from the unfused
    schedule;
  * dropout off: the bits are all ones and the multiplier is 1.

  kernel level (harness of tests/test_layer_ss_kernels_gpu.py: NaN-filled arenas with canaries, that file's bounds): two launches back to
    back into separate output sets, byte-equal, no NaN, canaries intact, then every saved tensor against the fp64 reference.  ff 512 /
    1024 / 1536 / 2048 (nj = 1 .. 4: 1 has no earlier slice, 2 is the smallest at which the moved epilogue meets its buffer's previous
    reader, 3 and 4 write a buffer a linear2 slice has read); rows 19 / 17 / 16 / 13 / 1 (17 and 16: a second row tile with one valid row
    and with none) x memory rows 13 / 16 / 0 (0 = encoder layer); 1 and 2 layers, with and without the final norm; dropout 0.3 and 0.0.
  fused against the unfused schedule: test_layer_ss_overlap_gpu's comparison and tolerances, for the benchmark's shape and one per ff.
  eager step against launch-list replay: bitwise equal losses and parameters over three steps, a fresh mask in each."""
import pytest
import torch

import vct_oracle as O
import test_layer_ss_overlap_gpu as OV
from helpers import build_model
from test_layer_ss_gpu import _mc
from test_layer_ss_kernels_gpu import Arena, Fwd

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@pytest.fixture(scope="module")
def ops():
    from vct_amd import ops as _ops
    return _ops


def _id(c):
    return "-".join(f"{k}{v}" for k, v in c.items())


# every (rows, memory rows) pair; every ff with both row-tile counts, both depths, both settings of the final norm and of dropout
KERNEL_CASES = [
    dict(L=19, Lm=13, ff=2048, n_layers=2, last=True, p=0.3),       # the benchmark's decoder stack
    dict(L=19, Lm=16, ff=1024, n_layers=1, last=False, p=0.0),
    dict(L=19, Lm=0, ff=1536, n_layers=2, last=False, p=0.3),
    dict(L=17, Lm=13, ff=1024, n_layers=2, last=False, p=0.3),
    dict(L=17, Lm=16, ff=1536, n_layers=1, last=True, p=0.3),
    dict(L=17, Lm=0, ff=2048, n_layers=1, last=True, p=0.0),
    dict(L=16, Lm=13, ff=1536, n_layers=2, last=True, p=0.0),
    dict(L=16, Lm=16, ff=2048, n_layers=1, last=False, p=0.3),
    dict(L=16, Lm=0, ff=1024, n_layers=2, last=True, p=0.3),
    dict(L=13, Lm=13, ff=512, n_layers=2, last=True, p=0.3),
    dict(L=13, Lm=16, ff=2048, n_layers=2, last=False, p=0.0),
    dict(L=13, Lm=0, ff=2048, n_layers=2, last=True, p=0.3),        # the benchmark's encoder stack
    dict(L=1, Lm=13, ff=1024, n_layers=1, last=True, p=0.3),
    dict(L=1, Lm=16, ff=1536, n_layers=2, last=False, p=0.3),
    dict(L=1, Lm=0, ff=512, n_layers=2, last=False, p=0.0),
    dict(L=19, Lm=13, ff=512, n_layers=1, last=False, p=0.0),
    dict(L=17, Lm=0, ff=512, n_layers=1, last=True, p=0.3),
    dict(L=19, Lm=0, ff=1024, n_layers=1, last=True, p=0.0),
    dict(L=13, Lm=0, ff=1024, n_layers=1, last=False, p=0.3),
]


@pytest.mark.parametrize("case", KERNEL_CASES, ids=_id)
def test_two_launches_byte_equal_and_every_saved_tensor_against_fp64(ops, case):
    f = Fwd(ops, B=3, mask="ids" if case["Lm"] else "raw" if case["L"] > 1 else "byte", **case)
    arenas = [Arena(16 << 20), Arena(16 << 20)]                 # NaN everywhere (0xFF bytes) before the launches
    descs = [f.descs(ar) for ar in arenas]
    for d in descs:                                              # the second launch follows the first with no synchronisation between
        ops.layer_ss_fwd(d)
    torch.cuda.synchronize()
    for ar in arenas:
        ar.check()                                               # every element of every output finite, every canary intact
    assert torch.equal(arenas[0].buf, arenas[1].buf), "two back-to-back launches gave different bytes"
    f.check()                                                    # every saved tensor against the fp64 reference (masks included: check_zeros)


# decoder rows = S - 1, memory rows = encoder rows = T + 1
SCHEDULE_CASES = [
    dict(T=12, S=20, ff=2048, enc=2, dec=2),      # the benchmark's shape: 19 rows, 13 memory rows
    dict(T=15, S=18, ff=512, enc=1, dec=2),
    dict(T=15, S=17, ff=1024, enc=2, dec=1),
    dict(T=12, S=18, ff=1536, enc=1, dec=1),
    dict(T=15, S=14, ff=2048, enc=1, dec=1),
]


@pytest.mark.parametrize("case", SCHEDULE_CASES, ids=_id)
def test_fused_equals_unfused_every_saved_tensor(case):
    """The comparison of tests/test_layer_ss_overlap_gpu.py, at its tolerances, dropout 0.3: every saved tensor behind a dropout site
    carries the mask, so one wrong keep bit is a whole element's difference."""
    OV.test_fused_equals_unfused_every_saved_tensor(case)


def test_eager_step_equals_launch_list_replay():
    from vct_amd.trainer import CaptionTrainer, FusedAdam
    V = 900
    mc = _mc(enc=1, dec=2, ff=1024, dropout=0.3)
    cfg = O.cfg_from_model_config(mc, V)
    p = O.init_params(cfg, seed=2)
    fe, mk, ii = (torch.from_numpy(a).to(DEV) for a in O.synthetic_batch(3, 12, 512, 20, V, seed=4))
    res = {}
    for launch_list in (False, True):
        m = build_model(mc, V, DEV, BF, p)
        m.train(); m._seed.fill_(11)
        tr = CaptionTrainer(m, FusedAdam(m, lr=1e-4), launch_list=launch_list)
        losses = torch.cat([tr.step(fe, mk, ii).clone() for _ in range(3)])      # the list is recorded in the first step and replayed after it
        torch.cuda.synchronize()
        if launch_list:
            assert len(tr._lists) == 1
        res[launch_list] = (losses, m.flat_params.clone())
    assert torch.equal(res[False][0], res[True][0]) and torch.equal(res[False][1], res[True][1])
    assert len(set(res[True][0].tolist())) == 3                 # a fresh dropout mask every step
