"""Caption metrics without a device: metrics.CaptionMetrics (host fp64) against hand-worked cases and against the independent
reference tests/capmetric_ref.py, the CIDEr term's identity with rewards.CiderD, tokenisation, the table layout, the C-ABI
refusals of the three entry points (codes before any launch) and the early-stopping score."""
import ctypes

import numpy as np
import pytest

import capmetric_ref as R

# host fp64 against host fp64: the same few hundred terms summed in another order
FP64_TOL = 1e-12

W = {w: i for i, w in enumerate("the cat is on mat there a dog sat".split())}


def _ids(s):
    return [W[w] for w in s.split()]


def _cm(refs, **kw):
    from vct_amd.metrics import CaptionMetrics
    return CaptionMetrics(refs, **kw)


def _close(a, b, tol=FP64_TOL):
    return abs(a - b) <= tol * max(abs(a), abs(b))


def test_clipping_hand_worked():
    """'the' x 7 against the two classic references: unigram clipping at 2, nothing above; closest reference length 7."""
    refs = {"v": [_ids("the cat is on the mat"), _ids("there is a cat on the mat")], "w": [_ids("a dog sat")]}
    pc = _cm(refs).per_caption({"v": _ids("the the the the the the the")})
    row = pc["counts"][0].tolist()
    assert row[0] == 7 and row[1] == 7 and row[2:6] == [2, 0, 0, 0] and row[6:10] == [7, 6, 5, 4] and row[10] == 2 and row[11] == 0
    prec, rec, f = pc["rouge"][0]
    assert prec == 2 / 7 and rec == 2 / 6
    assert _close(f, (1 + 1.44) * prec * rec / (rec + 1.44 * prec))


def test_candidate_equal_to_a_reference():
    refs = {"v": [_ids("the cat is on the mat")], "w": [_ids("a dog sat on the mat")]}
    cm = _cm(refs)
    out = cm.score({"v": _ids("the cat is on the mat"), "w": _ids("a dog sat on the mat")})
    for k in range(1, 5):
        assert abs(out[f"Bleu_{k}"] - 1.0) < 1e-9
    assert out["ROUGE_L"] == 1.0
    assert out["CIDEr"] > 0 and _close(out["sum"], out["Bleu_4"] + out["ROUGE_L"] + out["CIDEr"])


def test_reflen_tie_goes_to_the_shorter_reference():
    refs = {"v": [[1, 2, 3, 4, 5, 6, 7], [1, 2, 3], [1, 2, 3, 4, 5, 6, 7, 8, 9]]}       # |7 - 5| == |3 - 5|
    assert _cm(refs).per_caption({"v": [1, 2, 3, 4, 5]})["counts"][0, 1] == 3
    refs = {"v": [[1] * 8, [1] * 4]}
    assert _cm(refs).per_caption({"v": [1] * 6})["counts"][0, 1] == 4


def test_short_empty_and_unreferenced():
    refs = {"v": [[1, 2, 3, 4, 5], [2, 3]], "none": [], "w": [[7, 8, 9]]}
    cm = _cm(refs, end_id=102)
    pc = cm.per_caption({"v": [2, 3, 102, 4, 5], "none": [1, 2, 3], "w": [102, 7, 8]})
    short, none, empty = (pc["counts"][i].tolist() for i in range(3))
    assert short == [2, 2, 2, 1, 0, 0, 2, 1, 0, 0, 2, 0]                               # guesses of a 2-token candidate: 2, 1, 0, 0
    assert pc["rouge"][0].tolist() == [1.0, 1.0, 1.0]
    assert none == [0] * 12 and pc["rouge"][1].tolist() == [0.0] * 3 and pc["cider"][1] == 0.0
    assert empty == [0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0] and pc["rouge"][2].tolist() == [0.0] * 3 and pc["cider"][2] == 0.0
    out = cm.score({"v": [2, 3, 102, 4, 5], "none": [1, 2, 3], "w": [102, 7, 8]})
    assert _close(out["ROUGE_L"], 1.0 / 3.0)                                           # the unreferenced video counts in the mean
    assert all(np.isfinite(v) for v in out.values())


def test_end_token_is_dropped_and_the_tail_ignored():
    refs = {"v": [[1, 2, 3, 4]], "w": [[5, 6]]}
    cm = _cm(refs, end_id=102)
    a = cm.per_caption({"v": [1, 2, 3, 102, 1, 2, 3, 4]})
    b = cm.per_caption({"v": [1, 2, 3]})
    assert a["counts"].tolist() == b["counts"].tolist() and a["rouge"].tobytes() == b["rouge"].tobytes() and a["cider"].tobytes() == b["cider"].tobytes()
    assert a["counts"][0, 0] == 3
    whole = _cm(refs).per_caption({"v": [1, 2, 3, 102]})                                # no end id: the row is taken whole
    assert whole["counts"][0, 0] == 4


@pytest.mark.parametrize("seed", [0, 1])
def test_host_scorer_against_the_reference(seed):
    """64 videos x 1..7 references over a 12-word vocabulary: integer rows equal, floats within 1e-12."""
    refs, cands = R.random_corpus(seed)
    cm = _cm(refs)
    pc = cm.per_caption(cands)
    want, rows, rouge, ciders = R.score(refs, cands)
    assert pc["vids"] == list(cands)
    assert pc["counts"].tolist() == rows
    assert pc["counts"][:, 2].sum() < pc["counts"][:, 6].sum() and pc["counts"][:, 2].sum() > 0        # clipping happens
    for got, tri in zip(pc["rouge"], rouge):
        assert got[0] == tri[0] and got[1] == tri[1] and _close(got[2], tri[2])
    for got, c in zip(pc["cider"], ciders):
        assert _close(got, c) and (c != 0.0 or got == 0.0)
    out = cm.score(cands)
    assert set(out) == {"Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4", "ROUGE_L", "CIDEr", "sum"}
    for k, v in want.items():
        assert _close(out[k], v), (k, out[k], v)
    assert 0 < out["Bleu_4"] < out["Bleu_1"] < 1 and 0 < out["ROUGE_L"] < 1 and out["CIDEr"] > 0


def test_brevity_penalty_both_sides():
    refs = {"v": [[1, 2, 3, 4, 5, 6]], "w": [[1, 2, 3, 4, 5, 6]]}
    cm = _cm(refs)
    short = cm.score({"v": [1, 2, 3, 4], "w": [1, 2, 3, 4]})                           # ratio 8 / 12 < 1
    long_ = cm.score({"v": [1, 2, 3, 4, 5, 6, 1, 2], "w": [1, 2, 3, 4, 5, 6]})           # ratio 14 / 12 >= 1: no penalty
    assert _close(short["Bleu_1"], np.exp(1 - 12 / 8), 1e-9)
    assert _close(long_["Bleu_1"], 12 / 14, 1e-9)
    for out, cands in ((short, {"v": [1, 2, 3, 4], "w": [1, 2, 3, 4]}), (long_, {"v": [1, 2, 3, 4, 5, 6, 1, 2], "w": [1, 2, 3, 4, 5, 6]})):
        want = R.score(refs, cands)[0]
        assert all(_close(out[k], want[k]) for k in want)


def test_cider_term_is_rewards_ciderd():
    """The CIDEr term is rewards.CiderD over the same references with an end id that never occurs -- the same code, so bitwise."""
    from vct_amd.rewards import CiderD
    refs, cands = R.random_corpus(3)
    cm = _cm(refs)
    cd = CiderD(refs, n=4, sigma=6.0, end_id=10 ** 9)
    pc = cm.per_caption(cands)
    want = np.asarray([cd.score(c, v) for v, c in cands.items()], np.float64)
    assert pc["cider"].tobytes() == want.tobytes() and (want > 0).sum() > len(want) // 2
    assert cm.score(cands)["CIDEr"] == sum(float(x) for x in want) / len(want)


def test_normalize_caption_and_word_table():
    from vct_amd.metrics import WordTable, normalize_caption
    assert normalize_caption("A man is  Playing, the guitar.") == ["a", "man", "is", "playing", "the", "guitar"]
    assert normalize_caption("Wait... what?! -- (a 'dog') ; well-known: \"yes\"") == ["wait", "what", "a", "dog", "well-known", "yes"]
    assert normalize_caption("he doesn't run") == ["he", "doesn't", "run"]              # PTB would split the contraction: documented
    assert normalize_caption("  ") == [] and normalize_caption(" - ' . ") == []
    t = WordTable()
    a = t.encode("The cat sat.")
    assert a == [0, 1, 2] and t.encode("the CAT") == [0, 1] and len(t) == 3
    b = t.encode("the zebra sat zebra")                                               # an unseen candidate word: a fresh id, one per word
    assert b == [0, 3, 2, 3] and len(t) == 4
    refs = {"v": [a], "w": [t.encode("cat")]}
    pc = _cm(refs).per_caption({"v": b})
    assert pc["counts"][0, 2:6].tolist() == [2, 0, 0, 0]


def test_device_tables_layout():
    refs, _ = R.random_corpus(5, n_videos=9)
    refs["empty"] = []
    cm = _cm(refs, end_id=102)
    T = cm.device_tables()
    for k, dt in (("vid_ref_ptr", np.int32), ("ref_tok_ptr", np.int32), ("ref_tok", np.int32), ("ref_len", np.int32),
                  ("table_keys", np.int32), ("table_idf", np.float64), ("ent_w", np.float64), ("ref_norm", np.float64)):
        assert T[k].dtype == dt and T[k].flags["C_CONTIGUOUS"], k
    assert T["end_id"] == 102 and T["beta_sq"] == 1.2 * 1.2 == 1.44 and T["n"] == 4 and T["two_sigma_sq"] == 72.0
    assert _cm(refs).device_tables()["end_id"] == -1
    n_ref = sum(len(rs) for rs in refs.values())
    assert T["vid_ref_ptr"].shape == (len(refs) + 1,) and T["vid_ref_ptr"][-1] == n_ref and T["ref_tok_ptr"].shape == (n_ref + 1,)
    assert T["ref_tok_ptr"][0] == 0 and T["ref_tok_ptr"][-1] == T["ref_tok"].shape[0]
    for vid, rs in refs.items():
        row = T["vid_row"][vid]
        r0, r1 = T["vid_ref_ptr"][row], T["vid_ref_ptr"][row + 1]
        assert r1 - r0 == len(rs)
        for r, want in zip(range(r0, r1), rs):
            assert T["ref_tok"][T["ref_tok_ptr"][r]:T["ref_tok_ptr"][r + 1]].tolist() == want and T["ref_len"][r] == len(want)
    with pytest.raises(ValueError, match="reference ids"):
        _cm({"v": [[1, -3]]})


def test_early_stopping_score():
    from vct_amd import evaluate
    refs, cands = R.random_corpus(2, n_videos=8)
    out = _cm(refs).score(cands)
    s = evaluate.metric_earlystop_score(out)
    assert s == out["sum"] == out["Bleu_4"] + out["ROUGE_L"] + out["CIDEr"] and isinstance(s, float)
    assert "three" in evaluate.metric_earlystop_score.__doc__.lower() and "METEOR" in evaluate.eval_metrics.__doc__


# ---- the C-ABI boundary -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from vct_amd import _lib
    return _lib.load()


def _desc(p, **kw):
    from vct_amd import _lib
    d = _lib.CapMetricDesc()
    d.C, d.L, d.stride_c, d.stride_l, d.end_id, d.n_videos, d.beta_sq = 3, 8, 9, 1, 102, 2, 1.44
    for f in ("ids", "vid_rows", "vid_ref_ptr", "ref_tok_ptr", "ref_tok", "counts", "rouge"):
        setattr(d, f, p)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _cider_desc(p, **kw):
    from vct_amd import _lib
    d = _lib.CiderDesc()
    d.B, d.N, d.L, d.n = 2, 1, 8, 4
    d.stride_b, d.stride_n, d.stride_l, d.end_id = 9, 0, 1, 102
    d.log_nvid, d.two_sigma_sq, d.n_videos, d.table_cap = 1.0, 72.0, 2, 16
    for f in ("ids", "vid_rows", "table_keys", "table_idf", "vid_ref_ptr", "ref_len", "ref_norm", "ref_ent_ptr", "ent_keys", "ent_w"):
        setattr(d, f, p)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_entry_points_refuse_before_any_launch(lib):
    """Dummy host pointers: every call below must return its code without a launch.  Shape refusals are tried on descriptors whose
    outputs are NULL as well (VCT_E_ARG, checked later), so a missing shape check shows as the wrong code."""
    ARG, SHAPE, ALIGN = -1, -2, -3
    raw = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(raw) + 15) & ~15
    assert lib.vct_capmetric_counts(None, None) == ARG
    assert lib.vct_capmetric_counts(_desc(p, counts=None), None) == ARG and lib.vct_capmetric_counts(_desc(p, rouge=None), None) == ARG
    assert lib.vct_capmetric_counts(_desc(p, ids=None), None) == ARG and lib.vct_capmetric_counts(_desc(p, ref_tok=None), None) == ARG
    assert lib.vct_capmetric_counts(_desc(p, C=0, counts=None), None) == SHAPE
    assert lib.vct_capmetric_counts(_desc(p, L=65, counts=None), None) == SHAPE and lib.vct_capmetric_counts(_desc(p, L=-1, counts=None), None) == SHAPE
    assert lib.vct_capmetric_counts(_desc(p, L=64, counts=None), None) == ARG and lib.vct_capmetric_counts(_desc(p, L=0, counts=None), None) == ARG
    assert lib.vct_capmetric_counts(_desc(p, beta_sq=0.0), None) == ARG
    assert lib.vct_capmetric_counts(_desc(p, rouge=p + 4), None) == ALIGN and lib.vct_capmetric_counts(_desc(p, ids=p + 4), None) == ALIGN
    assert lib.vct_capmetric_counts(_desc(p, counts=p + 2), None) == ALIGN
    # vct_cider_d_eval: vct_cider_d's refusals, reward optional, score required and 8-byte aligned
    assert lib.vct_cider_d_eval(None, p, None) == ARG
    assert lib.vct_cider_d_eval(_cider_desc(p), None, None) == ARG
    assert lib.vct_cider_d_eval(_cider_desc(p, ent_w=None), p, None) == ARG
    assert lib.vct_cider_d_eval(_cider_desc(p, B=0), None, None) == SHAPE and lib.vct_cider_d_eval(_cider_desc(p, L=65), None, None) == SHAPE
    assert lib.vct_cider_d_eval(_cider_desc(p), p + 4, None) == ALIGN
    assert lib.vct_cider_d_eval(_cider_desc(p, table_idf=p + 4), p, None) == ALIGN
    # vct_capmetric_finish
    assert lib.vct_capmetric_finish(3, None, p, p, p, None) == ARG and lib.vct_capmetric_finish(3, p, None, p, p, None) == ARG
    assert lib.vct_capmetric_finish(3, p, p, p, None, None) == ARG
    assert lib.vct_capmetric_finish(0, p, p, None, p, None) == SHAPE and lib.vct_capmetric_finish(-4, p, p, p, p, None) == SHAPE
    assert lib.vct_capmetric_finish(3, p, p + 4, None, p, None) == ALIGN and lib.vct_capmetric_finish(3, p, p, p + 4, p, None) == ALIGN
    assert lib.vct_capmetric_finish(3, p, p, None, p + 4, None) == ALIGN


def test_count_columns_and_binding():
    """metrics' column count against the binding's (and that against the header: tests/test_abi_cpu.py)."""
    from vct_amd import _lib, metrics
    assert metrics.COUNT_COLS == _lib.CAPMETRIC_COUNT_COLS
    assert {"vct_capmetric_counts", "vct_cider_d_eval", "vct_capmetric_finish"} <= set(_lib.exported_symbols()) and _lib.ABI_VERSION == 16
