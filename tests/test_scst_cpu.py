"""Self-critical sequence training, host side: CIDEr-D on token ids against the independent restatement (tests/scst_ref.py) and
hand-worked cases, the leave-one-out advantages, the C ABI of vct_wce_loss / vct_group_sum (argument errors are codes, no device
work) and the refusals of CaptionTrainer.scst_step."""
import ctypes
import math

import numpy as np
import pytest
import torch

import scst_ref as R
from helpers import build_model, golden_params, load_golden, model_config_of
import vct_oracle as O

END = 102


# ---- CIDEr-D ------------------------------------------------------------------------------------------------------------------------
def _random_corpus(seed, nvid=5, nref=3, vocab=9):
    rng = np.random.default_rng(seed)
    refs = {}
    for v in range(nvid):
        rs = []
        for _ in range(nref):
            ln = int(rng.integers(2, 13))
            body = [int(t) for t in rng.integers(1, vocab + 1, ln - 1)]
            rs.append(body + [END])
        refs[f"v{v}"] = rs
    return rng, refs


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_cider_d_matches_the_restatement_on_random_corpora(seed):
    from vct_amd.rewards import CiderD
    rng, refs = _random_corpus(seed)
    scorer = CiderD(refs)
    vids = list(refs)
    B, N, L = len(vids), 4, 14
    ids = np.zeros((B, N, L), np.int64)
    ids[:, :, 0] = 101
    for b in range(B):
        for n in range(N):
            ln = int(rng.integers(2, 13))
            row = [int(t) for t in rng.integers(1, 10, ln - 1)]
            if n == 0:                                  # one candidate per video close to a reference: scores well above 0
                row = list(refs[vids[b]][0][:-1])
                row[len(row) // 2] = int(rng.integers(1, 10))
            if n != 3:                                  # sample 3 never ends
                row = row + [END]
            ids[b, n, 1:1 + len(row)] = row             # pads (0) behind the end token, as the sampler leaves them
            if n == 3:
                ids[b, n, 1 + len(row):] = rng.integers(1, 10, L - 1 - len(row))
    got = scorer(torch.from_numpy(ids), vids)
    assert got.shape == (B, N) and got.dtype == np.float32
    want = np.array([[R.cider_d(ids[b, n, 1:].tolist(), vids[b], refs) for n in range(N)] for b in range(B)])
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-7)
    assert got.max() > 1.0 and (got > 0).sum() >= B and np.isfinite(got).all() and got.min() >= 0.0     # not a comparison of zeros
    for b in range(B):                                  # the scalar entry point agrees with the table
        assert scorer.score(ids[b, 1, 1:].tolist(), vids[b]) == pytest.approx(float(want[b, 1]), rel=1e-6, abs=1e-7)


def test_cider_d_hand_worked_cases():
    from vct_amd.rewards import CiderD
    refs = {"a": [[5, 6, 7, 8, END]], "b": [[9, 10, 11, 12, END]]}
    s = CiderD(refs)
    # a candidate equal to its video's only reference: every order's cosine is 1, no length penalty -> 10
    assert s.score([5, 6, 7, 8, END], "a") == pytest.approx(10.0, rel=1e-12)
    assert s.score([5, 6, 7, 8, END, 0, 0], "a") == pytest.approx(10.0, rel=1e-12)       # cut after the end token
    # ... and scored against the OTHER video it shares only the end token, whose idf is log 2 - log 2 = 0
    assert s.score([5, 6, 7, 8, END], "b") == 0.0
    assert s.score([20, 21, 22], "a") == 0.0 and s.score([], "a") == 0.0 and s.score([END], "a") == 0.0
    # no end token: one token short of the reference.  Order k has 5 - k candidate n-grams, all among the reference's 5 - k + 1 (the
    # unigram END weighs 0), every weight log 2: cosines 1, 3 / (sqrt3 * 2), 2 / (sqrt2 * sqrt3), 1 / sqrt2; penalty exp(-1 / 72)
    want = 10.0 * math.exp(-1.0 / 72.0) * (1.0 + math.sqrt(3) / 2 + math.sqrt(2.0 / 3.0) + 1 / math.sqrt(2)) / 4
    assert s.score([5, 6, 7, 8], "a") == pytest.approx(want, rel=1e-12)
    assert s.score([5, 6, 7, 8], "a") == pytest.approx(R.cider_d([5, 6, 7, 8], "a", refs), rel=1e-12)
    assert s.score([5, 6, 7, 8], "a") < s.score([5, 6, 7, 8, END], "a")                  # ending is rewarded
    # the length penalty alone: with one reference it is a common factor of every order
    cand = [5, 6, 7, 8, 5, 6, 7, 8, END]                                                  # 4 tokens longer
    wide = CiderD(refs, sigma=1e9)
    assert wide.score(cand, "a") > 0
    assert s.score(cand, "a") == pytest.approx(wide.score(cand, "a") * math.exp(-16.0 / 72.0), rel=1e-9)
    # a single-video corpus: every idf is log 1 - log 1 = 0
    one = CiderD({"a": [[5, 6, 7, END], [5, 6, END]]})
    assert one.score([5, 6, 7, END], "a") == 0.0 and one.score([1, 2], "a") == 0.0
    assert (one(np.array([[[101, 5, 6, 7, END]]]), ["a"]) == 0).all()
    with pytest.raises(ValueError):
        s(np.zeros((2, 5), np.int64), ["a", "b"])


# ---- advantages ------------------------------------------------------------------------------------------------------------------------
def test_leave_one_out_advantages():
    from vct_amd.rewards import advantages
    rng = np.random.default_rng(3)
    r = rng.random((4, 5)).astype(np.float32)
    a = advantages(r, "mean_others")
    assert a.shape == (4, 5) and a.dtype == np.float32
    np.testing.assert_allclose(a.sum(1), 0.0, atol=1e-6)
    for b in range(4):
        for n in range(5):
            assert a[b, n] == pytest.approx(r[b, n] - np.delete(r[b], n).mean(), abs=1e-6)
    r2 = np.array([[0.25, 1.0], [3.0, -1.0]], np.float32)
    np.testing.assert_array_equal(advantages(r2, "mean_others"), np.array([[-0.75, 0.75], [4.0, -4.0]], np.float32))
    with pytest.raises(ValueError, match="num_samples >= 2"):
        advantages(r[:, :1], "mean_others")
    # a caller-supplied baseline per video
    base = np.array([0.5, 0.0, 1.0, 2.0])
    np.testing.assert_allclose(advantages(r, base), r - base[:, None].astype(np.float32), atol=1e-7)
    with pytest.raises(ValueError):
        advantages(r, base[:3])
    with pytest.raises(ValueError):
        advantages(r, "median")


# ---- C ABI -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from vct_amd import _lib
    return _lib.load()


def test_wce_loss_and_group_sum_argument_errors_are_codes(lib):
    """Every call returns before its first launch: dummy host pointers, no device."""
    from vct_amd import _lib
    OK_, ARG, SHAPE, ALIGN = 0, -1, -2, -3
    raw = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(raw) + 15) & ~15

    def wce(dtype=_lib.BF16, N=12, S=4, V=257, logits=p, ldl=264, labels=p, stride=5, pad=0, seq_w=p, loss=p, tok=p, dl=p, ld_dl=264,
            ws=p):
        return lib.vct_wce_loss(dtype, N, S, V, logits, ldl, labels, stride, pad, seq_w, loss, tok, dl, ld_dl, ws, None)
    assert wce(logits=None) == ARG and wce(labels=None) == ARG and wce(loss=None) == ARG and wce(ws=None) == ARG and wce(dtype=7) == ARG
    assert wce(N=13) == SHAPE and wce(N=0) == SHAPE and wce(S=0) == SHAPE and wce(V=0) == SHAPE          # N % S != 0, empty
    assert wce(ldl=257) == ALIGN and wce(ldl=256) == ALIGN and wce(logits=p + 4) == ALIGN                 # rows are 16-byte vectors
    assert wce(ld_dl=260) == ALIGN and wce(dl=p + 8) == ALIGN
    assert wce(dtype=_lib.F32, ldl=258, ld_dl=260) == ALIGN and wce(dtype=_lib.F32, ldl=260, ld_dl=258) == ALIGN
    assert wce(V=65537, ldl=65544, ld_dl=65544) == SHAPE and wce(ld_dl=65544) == SHAPE                    # wider than the register tile
    assert wce(dtype=_lib.F32, V=32769, ldl=32772, ld_dl=32772) == SHAPE
    assert wce(V=65537, ldl=65544, dl=None, ld_dl=0) == SHAPE                                             # forward only: same width limit

    def gs(dtype=_lib.BF16, B=2, G=3, R=5, d=64, src=p, out=p):
        return lib.vct_group_sum(dtype, B, G, R, d, src, out, None)
    assert gs(src=None) == ARG and gs(out=None) == ARG and gs(dtype=9) == ARG
    assert gs(G=0) == SHAPE and gs(G=-1) == SHAPE and gs(B=0) == SHAPE and gs(R=0) == SHAPE
    assert gs(d=0) == SHAPE and gs(d=60) == SHAPE and gs(dtype=_lib.F32, d=66) == SHAPE and gs(d=4) == SHAPE
    assert gs(src=p + 8) == ALIGN and gs(out=p + 4) == ALIGN
    assert OK_ == 0


# ---- scst_step refusals ----------------------------------------------------------------------------------------------------------------
class _ActiveExchange:
    active, world, group = True, 2, None


def _cpu_model():
    z = load_golden("tiny_train.npz")
    mc = model_config_of(z)
    cfg = O.cfg_from_model_config(mc, int(z["vocab"]))
    m = build_model(mc, int(z["vocab"]), "cpu", torch.float32, golden_params(z, cfg))
    return m, torch.from_numpy(z["feats"]), torch.from_numpy(z["mask"])


def test_scst_step_refuses_before_any_device_work():
    from vct_amd.trainer import CaptionTrainer
    m, feats, mask = _cpu_model()
    m.train()
    opt = torch.optim.Adam([m.flat_params], lr=1e-4)

    def reward_fn(ids, vids):
        raise AssertionError("the step must refuse before it samples")
    for kw in (dict(use_graph=True), dict(launch_list=True), dict(exchange=_ActiveExchange())):
        tr = CaptionTrainer(m, opt, **kw)        # the caption task's constructor takes them as before
        with pytest.raises(NotImplementedError, match="eager|single-process"):
            tr.scst_step(feats, mask, reward_fn, num_samples=2)
    tr = CaptionTrainer(m, opt)
    with pytest.raises(ValueError, match="num_samples >= 2"):
        tr.scst_step(feats, mask, reward_fn, num_samples=1)
    with pytest.raises(ValueError, match="baseline"):
        tr.scst_step(feats, mask, reward_fn, num_samples=2, baseline="median")
    m.mode("match")
    with pytest.raises(ValueError, match="caption task"):
        tr.scst_step(feats, mask, reward_fn, num_samples=2)
    m.mode("caption")
    # the model-level entry points check their id table in Python
    with pytest.raises(ValueError, match="ids must be int64"):
        m.train_step_kernels_scst(feats, mask, torch.zeros(5, 6, dtype=torch.int64), torch.zeros(5), num_samples=2)
    with pytest.raises(ValueError, match="ids must be int64"):
        m.score_captions([feats], [mask], torch.zeros(feats.shape[0], 6, dtype=torch.int32))
