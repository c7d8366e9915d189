"""The fused stack forward with its saved-tensor copies carried inside the K loop of the product that follows them
(csrc/vct_layer_ss_core.h: panel_to_global_slice, wave_gemm8_cb).  A copy that reads its LDS slot after the slot changed its role, or a
product that starts before the copy it displaced was issued, shows up as a saved tensor that differs from the unfused schedule, from a
second identical launch, or from the fp64 reference.

  * fused against the unfused kernel schedule, every saved tensor, dropout 0.3, batch 3: decoder rows 19 / 17 / 16 / 13 / 1 x memory
    (= encoder) rows 13 / 16, ff 512 (one chunk: no pipelined callback) / 1024 / 2048, stacks of 1 and 2 layers, encoder and decoder.
    Criteria "equal": those of tests/test_layer_ss_gpu.py::test_fused_equals_unfused_schedule, unchanged.  The model always has the
    stack-final norm, so the unfused schedule cannot run without it: the cases WITHOUT the final norm run at kernel level below.
  * hazards, at kernel level (harness of tests/test_layer_ss_kernels_gpu.py: NaN-filled arenas with canaries): the same launch twice on
    one stream, back to back, into two separate NaN-filled output sets -- byte-identical, no NaN in any row, canaries intact -- and the
    same outputs against the fp64 reference under that file's bounds; with and without the final norm.
  * one training step run eagerly and replayed from a recorded launch list: bitwise equal losses and parameters."""
import pytest
import torch

import vct_oracle as O
from helpers import build_model, rel
from test_layer_ss_gpu import _fuse, _mc
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


# decoder rows = S - 1, memory rows = encoder rows = T + 1: every (rows, memory rows) pair; every ff and both depths with each row count
SCHEDULE_CASES = [
    dict(T=12, S=20, ff=2048, enc=2, dec=2),      # the benchmark's shape: 19 rows, 13 memory rows
    dict(T=15, S=20, ff=512, enc=1, dec=1),
    dict(T=12, S=18, ff=1024, enc=1, dec=2),
    dict(T=15, S=18, ff=2048, enc=2, dec=1),
    dict(T=15, S=17, ff=1024, enc=2, dec=2),
    dict(T=12, S=17, ff=512, enc=1, dec=1),
    dict(T=12, S=14, ff=2048, enc=1, dec=1),
    dict(T=15, S=14, ff=512, enc=2, dec=2),
    dict(T=15, S=2, ff=1024, enc=1, dec=2),
    dict(T=12, S=2, ff=2048, enc=2, dec=1),
]


def _id(c):
    return "-".join(f"{k}{v}" for k, v in c.items())


@pytest.mark.parametrize("case", SCHEDULE_CASES, ids=_id)
def test_fused_equals_unfused_every_saved_tensor(case):
    V, B, T, S = 311, 3, case["T"], case["S"]
    mc = _mc(enc=case["enc"], dec=case["dec"], ff=case["ff"], dropout=0.3)
    cfg = O.cfg_from_model_config(mc, V)
    p = O.init_params(cfg, seed=5)
    f, mk, ids = O.synthetic_batch(B, T, 512, S, V, seed=S, ragged=True)
    feats, mask, idt = (torch.from_numpy(a).to(DEV) for a in (f, mk, ids))
    runs = {}
    old = _fuse(True)
    try:
        for fused in (True, False):
            _fuse(fused)
            m = build_model(mc, V, DEV, BF, p)
            m.train(); m._seed.fill_(4242)
            if fused:
                assert m.cap_decoder._engine()._ss_ok(S - 1, T + 1, B) and m.video_encoder._engine()._ss_ok(T + 1, 0, B)
            loss, _ = m._forward_loss(feats, mask, idt, True, want_logits=True)
            acts = {}
            for eng, pre in ((m.video_encoder._engine(), "enc."), (m.cap_decoder._engine(), "dec.")):
                for k, t in eng.cur.t.items():
                    if isinstance(k, str) and torch.is_tensor(t) and t.is_floating_point() and k not in ("logits", "dlogits", "row_ws", "loss"):
                        acts[pre + k] = t.float().clone()
            m._backward()
            runs[fused] = (float(loss), acts, m._ps.gflat.clone())
    finally:
        _fuse(old)
    (l1, a1, g1), (l0, a0, g0) = runs[True], runs[False]
    assert abs(l1 - l0) < 2e-3 * abs(l0)
    saved = [k for k in a0 if k in a1 and a0[k].shape == a1[k].shape]
    assert len(saved) >= 10 * (case["enc"] + case["dec"]), sorted(a0)
    for k in saved:
        assert bool(torch.isfinite(a1[k]).all()), k
        if k.endswith("mean"):
            assert float((a1[k] - a0[k]).abs().max()) < 5e-3, k
            continue
        tol = 3e-2 if k.endswith("rstd") else 2.5e-2
        assert rel(a1[k], a0[k]) < tol, (k, rel(a1[k], a0[k]))
    assert rel(g1, g0) < 3e-2


# kernel level: rows x ff x depth x final norm, encoder (Lm = 0) and decoder; every launch draws dropout 0.3
HAZARD_CASES = [
    dict(L=19, Lm=13, ff=2048, n_layers=2, last=True),
    dict(L=19, Lm=16, ff=512, n_layers=1, last=False),
    dict(L=17, Lm=13, ff=1024, n_layers=2, last=False),
    dict(L=16, Lm=16, ff=2048, n_layers=1, last=True),
    dict(L=13, Lm=13, ff=512, n_layers=2, last=True),
    dict(L=1, Lm=16, ff=1024, n_layers=2, last=False),
    dict(L=19, Lm=0, ff=1024, n_layers=2, last=False),
    dict(L=17, Lm=0, ff=512, n_layers=1, last=True),
    dict(L=16, Lm=0, ff=2048, n_layers=2, last=True),
    dict(L=13, Lm=0, ff=2048, n_layers=2, last=False),
    dict(L=13, Lm=0, ff=1024, n_layers=1, last=True),
    dict(L=1, Lm=0, ff=512, n_layers=2, last=False),
]


@pytest.mark.parametrize("case", HAZARD_CASES, ids=_id)
def test_back_to_back_launches_into_nan_filled_outputs(ops, case):
    f = Fwd(ops, B=3, p=0.3, mask="ids" if case["Lm"] else "raw" if case["L"] > 1 else "byte", **case)
    arenas = [Arena(16 << 20), Arena(16 << 20)]                 # NaN everywhere (0xFF bytes) before the launches
    descs = [f.descs(ar) for ar in arenas]
    for d in descs:                                              # the second launch follows the first with no synchronisation between
        ops.layer_ss_fwd(d)
    torch.cuda.synchronize()
    for ar in arenas:
        ar.check()                                               # every element of every output finite, every canary intact
    assert torch.equal(arenas[0].buf, arenas[1].buf), "two back-to-back launches gave different bytes"
    f.check()                                                    # and every saved tensor against the fp64 reference


def test_eager_step_equals_launch_list_replay():
    from vct_amd.trainer import CaptionTrainer, FusedAdam
    V = 900
    mc = _mc(enc=2, dec=2, ff=2048, dropout=0.3)
    cfg = O.cfg_from_model_config(mc, V)
    p = O.init_params(cfg, seed=1)
    fe, mk, ii = (torch.from_numpy(a).to(DEV) for a in O.synthetic_batch(16, 12, 512, 20, V, seed=3))
    res = {}
    for launch_list in (False, True):
        m = build_model(mc, V, DEV, BF, p)
        m.train(); m._seed.fill_(7)
        tr = CaptionTrainer(m, FusedAdam(m, lr=1e-4), launch_list=launch_list)
        losses = torch.cat([tr.step(fe, mk, ii).clone() for _ in range(3)])      # the list is recorded in the first step and replayed after it
        torch.cuda.synchronize()
        if launch_list:
            assert len(tr._lists) == 1
        res[launch_list] = (losses, m.flat_params.clone())
    assert torch.equal(res[False][0], res[True][0]) and torch.equal(res[False][1], res[True][1])
    assert len(set(res[True][0].tolist())) == 3                 # a fresh dropout mask every step
