"""Text-video retrieval evaluation without a GPU: the host scorer (vct_amd.retrieval.RetrievalMetrics, the definition) against
the independent fp64 restatement (tests/retrieval_ref.py), against a torch stable argsort and against hand-worked cases; the
restatement's interval check rejecting five wrong rankers; the conditions the GPU tests' generator must meet, on the restatement
alone; the refusals of the Python layer and the C-ABI boundary of vct_retrieval_ranks / vct_retrieval_workspace_bytes."""
import ctypes
import subprocess

import numpy as np
import pytest
import torch

import retrieval_ref as R


def _host(mode="plain", tau=None):
    from vct_amd.retrieval import RetrievalMetrics
    return RetrievalMetrics(mode, tau)


def _argsort_ranks(f, gt):
    """Ranks by sorting: position of the ground truth in a stable descending sort (ties keep index order)."""
    f = torch.from_numpy(np.asarray(f, np.float64))
    Nt, Nv = f.shape
    order_t = torch.argsort(-f, dim=1, stable=True)
    rt = [int((order_t[i] == int(gt[i])).nonzero()[0, 0]) + 1 for i in range(Nt)]
    order_v = torch.argsort(-f, dim=0, stable=True)
    rv = []
    for j in range(Nv):
        own = set(np.flatnonzero(np.asarray(gt) == j).tolist())
        rv.append(1 + next(k for k, i in enumerate(order_v[:, j].tolist()) if i in own) if own else 0)
    return np.asarray(rt), np.asarray(rv)


# ---- the host scorer -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,tau", R.GPU_MODES)
@pytest.mark.parametrize("shape", [(33, 2, 20), (67, 3, 20)])
def test_host_scorer_against_reference_and_argsort(shape, mode, tau):
    t, v, gt = R.make_case(*shape, seed=11, shuffle=True)
    h = _host(mode, tau)
    rt, rv = h.ranks(t, v, gt)
    ref = R.intervals(t, v, gt, mode, tau)
    assert np.array_equal(rt, ref["rt"]) and np.array_equal(rv, ref["rv"])
    f = R.scores(t, v, mode, tau)[1]
    assert np.allclose(h.scores(t, v), f, rtol=1e-12, atol=1e-15)
    at, av = _argsort_ranks(f, gt)
    assert np.array_equal(rt, at) and np.array_equal(rv, av)
    out = h.score(t, v, gt)
    for side, r in (("t2v", rt), ("v2t", rv)):
        st = R.stats(r)
        got = out[side]
        assert [got["R1"], got["R5"], got["R10"]] == [100.0 * x for x in st[:3]]
        assert (got["MedianR"], got["MeanR"], got["n"]) == (st[3], st[4], int(st[5]))
    assert out["rsum"] == sum(out[s][k] for s in ("t2v", "v2t") for k in ("R1", "R5", "R10"))


def test_hand_worked_three_videos_five_texts():
    v = np.eye(4, dtype=np.float32)[:3]                               # e0, e1, e2
    t = np.asarray([[3, 2, 1, 0], [3, 2, 1, 0], [3, 2, 1, 0], [0, 1, 2, 0], [1, 0, 0, 1]], np.float32)
    gt = [0, 1, 2, 1, 0]
    # rows ~ (3,2,1), (3,2,1), (3,2,1), (0,1,2), (1,0,0): the ground truth is 1st, 2nd, 3rd, 2nd, 1st in its row
    # columns: video 0 = {.80, .80, .80, 0, .71}, own {0, 4}: text 0 leads (nothing above, no tie with a lower index): 1
    #          video 1 = {.53, .53, .53, .45, 0}, own {1, 3}: text 1 ties with text 0, which has the lower index: 2
    #          video 2 = {.27, .27, .27, .89, 0}, own {2}: text 3 is above, texts 0 and 1 tie with lower indices: 4
    rt, rv = _host().ranks(t, v, gt)
    assert rt.tolist() == [1, 2, 3, 2, 1] and rv.tolist() == [1, 2, 4]
    assert [a.tolist() for a in R.ranks_from_matrix(R.scores(t, v)[1], gt)] == [[1, 2, 3, 2, 1], [1, 2, 4]]
    out = _host().score(t, v, gt)
    assert out["t2v"] == {"R1": 40.0, "R5": 100.0, "R10": 100.0, "MedianR": 2.0, "MeanR": 9 / 5, "n": 5}
    assert out["v2t"] == {"R1": 100.0 * (1 / 3), "R5": 100.0, "R10": 100.0, "MedianR": 2.0, "MeanR": 7 / 3, "n": 3}
    assert out["rsum"] == 40.0 + 100.0 + 100.0 + 100.0 * (1 / 3) + 100.0 + 100.0


def test_exact_ties_go_to_the_lower_index():
    t, v = np.ones((4, 8), np.float32), np.ones((3, 8), np.float32)   # every score is exactly 1
    gt = [2, 0, 1, 2]
    rt, rv = _host().ranks(t, v, gt)
    assert rt.tolist() == [3, 1, 2, 3]                                # text->video: the g videos before the ground truth win the tie
    assert rv.tolist() == [2, 3, 1]                                   # video->text: the best own text is the lowest-indexed one: 1, 2, 0
    rt2, rv2 = R.ranks_from_matrix(np.ones((4, 3)), gt)
    assert rt2.tolist() == [3, 1, 2, 3] and rv2.tolist() == [2, 3, 1]
    # in the dual softmax a column of equal scores keeps them equal
    rt3, rv3 = _host("dual_softmax", 0.5).ranks(t, v, gt)
    assert rt3.tolist() == [3, 1, 2, 3] and rv3.tolist() == [2, 3, 1]


def test_video_without_text_bad_gt_and_one_video():
    t, v, _ = R.make_case(3, 1, 8, seed=2)
    t = np.concatenate([t, t[:1], t[:1]])[:3]
    rt, rv = _host().ranks(t, v, [0, 0, 2])
    assert rv[1] == 0 and rv[0] > 0 and rv[2] > 0 and (rt > 0).all()
    out = _host().score(t, v, [0, 0, 2])
    assert out["v2t"]["n"] == 2 and out["t2v"]["n"] == 3
    rt, rv = _host().ranks(t, v, [0, 7, -1])                          # gt outside the videos: no query, no own text
    assert rt.tolist()[1:] == [0, 0] and rv.tolist()[1:] == [0, 0]
    assert R.ranks_from_matrix(R.scores(t, v)[1], [0, 7, -1])[0].tolist()[1:] == [0, 0]
    for mode, tau in R.GPU_MODES:
        rt, rv = _host(mode, tau).ranks(t, v[:1], [0, 0, 0])          # one video: every text ranks it first
        assert rt.tolist() == [1, 1, 1] and rv.tolist() == [1]


def test_median_of_even_and_odd_counts():
    from vct_amd.retrieval import rank_stats
    assert rank_stats([1, 3])["MedianR"] == 2.0 and rank_stats([3, 1, 10])["MedianR"] == 3.0
    assert rank_stats([0, 4, 0, 1, 2, 9])["MedianR"] == 3.0 and rank_stats([0, 4, 0, 1, 2, 9])["n"] == 4
    assert rank_stats([0, 0]) == {"R1": 0.0, "R5": 0.0, "R10": 0.0, "MedianR": 0.0, "MeanR": 0.0, "n": 0}
    assert R.stats([1, 3])[3] == 2.0 and R.stats([3, 1, 10])[3] == 3.0 and R.stats([0, 0]) == [0.0] * 6


# ---- the interval check rejects wrong rankers ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case67():
    t, v, gt = R.make_case(67, 3, 20, seed=5)
    return t, v, gt, {m: R.intervals(t, v, gt, m, tau) for m, tau in (("plain", None), ("dual_softmax", 0.5))}


def test_checker_accepts_the_right_ranks(case67):
    t, v, gt, refs = case67
    for mode, tau in (("plain", None), ("dual_softmax", 0.5)):
        ref = refs[mode]
        out = R.stats(ref["rt"]) + R.stats(ref["rv"])
        assert R.check(ref, ref["rt"], ref["rv"], out) == []
        assert R.check(ref, ref["lo_t"], ref["hi_v"]) == []


def _wrong_rankers(t, v, gt):
    s, f, _ = R.scores(t, v)
    dropped = f.copy()
    dropped[16:32, 16:32] = -np.inf
    yield "a dropped 16 x 16 block", "plain", R.ranks_from_matrix(dropped, gt)
    yield "a column shifted by one", "plain", R.ranks_from_matrix(np.roll(f, 1, axis=1), gt)
    yield ">= in place of >", "plain", R.ranks_from_matrix(f, gt, strict=False)
    z = s / 0.5
    wrong_axis = s * (np.exp(z) / np.exp(z).sum(axis=1, keepdims=True))
    yield "a softmax over the wrong axis", "dual_softmax", R.ranks_from_matrix(wrong_axis, gt)
    yield "a gt off by one", "plain", R.ranks_from_matrix(f, (np.asarray(gt) + 1) % v.shape[0])


def test_checker_rejects_wrong_rankers(case67):
    t, v, gt, refs = case67
    seen = []
    for what, mode, (rt, rv) in _wrong_rankers(t, v, gt):
        bad = R.check(refs[mode], rt, rv, R.stats(rt) + R.stats(rv))
        assert bad, what
        seen.append(what)
    assert len(seen) == 5


# ---- the generator of the GPU tests ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.GPU_SHAPES)
def test_generator_conditions(shape):
    """For every shape and mode of the GPU tests, with the seed the GPU tests use: at most 3 % of the queries (both directions
    together) have an ambiguous competitor (so the interval check is an equality check almost everywhere), and -- where the number of
    videos makes the question meaningful -- between 20 % and 80 % of the text queries have rank 1 (so neither `everything is rank
    1` nor a random ranker passes).  With one video every rank is 1 and with two a rank is one coin: the second condition is asked
    from 33 videos up.  retrieval_ref.make_case says how the noise range was chosen."""
    Nv, per, Dt = shape
    t, v, gt = R.make_case(Nv, per, Dt, seed=R.case_seed(shape))
    for mode, tau in R.GPU_MODES:
        ref = R.intervals(t, v, gt, mode, tau)
        amb_t, amb_v = float(np.mean(ref["amb_t"])), float(np.mean(ref["amb_v"]))
        amb = (np.count_nonzero(ref["amb_t"]) + np.count_nonzero(ref["amb_v"])) / (gt.size + Nv)
        share = float(np.mean(ref["rt"] == 1))
        print(f"[generator] {shape} {mode} tau={tau}: ambiguous t2v {amb_t:.4f} v2t {amb_v:.4f}, rank-1 share {share:.3f}")
        assert amb <= 0.03, (shape, mode, tau, amb_t, amb_v)
        if Nv >= 33:
            assert 0.2 <= share <= 0.8, (shape, mode, tau, share)


# ---- refusals of the Python layer ------------------------------------------------------------------------------------------------------
def test_python_refusals():
    from vct_amd import evaluate, ops
    from vct_amd.retrieval import DeviceRetrievalMetrics, RetrievalMetrics
    for bad in (dict(mode="cosine"), dict(mode="dual_softmax"), dict(mode="dual_softmax", tau=0.0), dict(mode="dual_softmax", tau=-1.0),
                dict(mode="plain", tau=0.5)):
        with pytest.raises(ValueError):
            RetrievalMetrics(**bad)
    with pytest.raises(ValueError, match="GPU"):
        RetrievalMetrics().to_device("cpu")
    h = RetrievalMetrics()
    with pytest.raises(ValueError):
        h.ranks(np.ones((3, 8)), np.ones((2, 4)), [0, 0, 0])
    with pytest.raises(ValueError):
        h.ranks(np.ones((3, 8)), np.ones((2, 8)), [0, 0])
    with pytest.raises(ValueError):
        h.ranks(np.ones((3, 8)), np.ones((0, 8)), [0, 0, 0])
    # shapes the kernels do not take: refused by the size query, before any device work
    assert ops.retrieval_workspace_bytes(10, 7, 16, "dual_softmax") > ops.retrieval_workspace_bytes(10, 7, 16, "plain") > 0
    assert ops.retrieval_workspace_bytes(1 << 20, 1 << 20, 1024, "plain") > 0
    for Nt, Nv, Dt in ((10, 7, 18), (10, 7, 1028), (10, 0, 16), (0, 7, 16), (10, 7, 0), ((1 << 20) + 1, 7, 16), (10, (1 << 20) + 1, 16)):
        with pytest.raises(ValueError, match="outside the kernels' range"):
            ops.retrieval_workspace_bytes(Nt, Nv, Dt)
    with pytest.raises(ValueError, match="mode"):
        ops.retrieval_workspace_bytes(10, 7, 16, "cosine")
    assert evaluate.retrieval_earlystop_score({"rsum": 123.5}) == 123.5


def test_model_refusals_stay_the_existing_ones():
    from helpers import build_model
    from hmm_ref import hmm_config, hmm_params
    import matching_ref as M
    from vct_amd import evaluate
    mc = hmm_config([48, 24], [2, 1])
    hm = build_model(mc, 131, "cpu", torch.float32, hmm_params(mc, 131, 5))
    feats = [torch.zeros(2, 5, 48), torch.zeros(2, 3, 24)]
    masks = [torch.zeros(2, 5, dtype=torch.bool), torch.zeros(2, 3, dtype=torch.bool)]
    with pytest.raises(NotImplementedError, match="hmme"):
        hm.embed_videos(feats, masks)
    with pytest.raises(NotImplementedError, match="hmme"):
        evaluate.eval_retrieval(hm, [])
    mc = M.matching_config([48], 64, None)
    nm = build_model(mc, 131, "cpu", torch.float32, M.matching_params(mc, 131, 5))
    with pytest.raises(ValueError, match="matching"):
        nm.embed_videos([torch.zeros(2, 5, 48)], [torch.zeros(2, 5, dtype=torch.bool)])
    with pytest.raises(ValueError, match="matching"):
        evaluate.eval_retrieval(nm, [])


# ---- the C-ABI boundary ----------------------------------------------------------------------------------------------------------------
NEW = ("vct_retrieval_ranks", "vct_retrieval_workspace_bytes")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from vct_amd import _lib
    return _lib.load()


def test_new_symbols_header_binding_and_library(lib):
    import test_abi_cpu as A
    from vct_amd import _lib
    decl = A.declared_symbols()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(l.split()[-1] for l in out.splitlines() if l.strip())
    for s in NEW:
        assert s in decl and s in _lib.exported_symbols() and s in exported, s
    assert sorted(set(decl)) == sorted(set(_lib.exported_symbols()))
    assert lib.vct_abi_version() == _lib.ABI_VERSION == 16              # additive: the version stays


def test_entry_point_refuses_before_any_launch(lib):
    """Dummy host pointers: every descriptor below is refused by a check that comes before the first launch, and the last one
    (a workspace one byte short) is the LAST check -- so a missing check shows as a wrong code, never as a launch."""
    from vct_amd import _lib
    ARG, SHAPE, ALIGN, WORKSPACE = -1, -2, -3, -4
    raw = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(raw) + 15) & ~15
    need = lib.vct_retrieval_workspace_bytes(10, 7, 16, 0)
    assert need > 0 and lib.vct_retrieval_workspace_bytes(10, 7, 16, 1) > need
    for args in ((10, 7, 18, 0), (10, 7, 1028, 0), (10, 0, 16, 0), (0, 7, 16, 0), (10, 7, 16, 2), (10, 7, 16, -1)):
        assert lib.vct_retrieval_workspace_bytes(*args) == 0, args

    def call(**kw):
        d = _lib.RetrievalDesc()
        d.Nt, d.Nv, d.Dt, d.mode = 10, 7, 16, 0
        d.text, d.ld_text, d.vid, d.ld_vid, d.gt = p, 16, p, 16, p
        d.ranks_t2v, d.ranks_v2t, d.out, d.workspace, d.workspace_bytes = p, p, p, p, need - 1
        for k, v in kw.items():
            setattr(d, k, v)
        return lib.vct_retrieval_ranks(d, None)
    assert lib.vct_retrieval_ranks(None, None) == ARG
    assert call() == WORKSPACE                                          # (the guard itself)
    for field in ("text", "vid", "gt", "ranks_t2v", "ranks_v2t", "out", "workspace"):
        assert call(**{field: None}) == ARG, field
    assert call(mode=2) == ARG and call(mode=-1) == ARG
    assert call(mode=1) == ARG and call(mode=0, tau=p) == ARG           # tau exactly in the dual-softmax mode
    assert call(mode=1, tau=p) == WORKSPACE
    assert call(phases=32) == ARG and call(phases=-1) == ARG and call(phases=8) == WORKSPACE
    assert call(Dt=18) == SHAPE and call(Dt=1028, ld_text=1028, ld_vid=1028) == SHAPE and call(Dt=0) == SHAPE
    assert call(Nv=0) == SHAPE and call(Nt=0) == SHAPE and call(Nt=(1 << 20) + 1) == SHAPE and call(Nv=(1 << 20) + 1) == SHAPE
    assert call(ld_text=12) == SHAPE and call(ld_vid=12) == SHAPE
    assert call(ld_text=18) == ALIGN and call(ld_vid=22) == ALIGN and call(ld_text=24, ld_vid=28) == WORKSPACE
    assert call(text=p + 4) == ALIGN and call(vid=p + 8) == ALIGN and call(workspace=p + 8) == ALIGN
    assert call(out=p + 4) == ALIGN and call(gt=p + 2) == ALIGN and call(ranks_t2v=p + 1) == ALIGN and call(ranks_v2t=p + 2) == ALIGN
    assert call(out=p + 8, gt=p + 4) == WORKSPACE
