"""The device reward without a device: rewards.CiderD.device_tables() against a restatement of the probe and a plain-loop scorer
that reads only the tables (tests/cider_dev_ref.py), the refusals of the table builder, and the C-ABI boundary of vct_cider_d /
vct_scst_advantages (codes before any launch)."""
import ctypes

import numpy as np
import pytest

import cider_dev_ref as D
import scst_ref as R

# host fp64 against host fp64 on bit-identical idf / r_w / norms: a few hundred terms summed in another order
FP64_TOL = 1e-12


def _cider(refs, **kw):
    from vct_amd.rewards import CiderD
    return CiderD(refs, end_id=D.END, **kw)


def _corpora():
    yield "small", D.small_corpus(), [D.small_candidates(D.small_corpus(), L) for L in D.SMALL_LENGTHS]
    yield "one_video", D.one_video_corpus(), [np.array([[[101, 3, 4, 5, D.END], [101, 4, 4, 6, 7]]], np.int64)]
    big = D.large_corpus()
    yield "large", big, [D.large_candidates(big)]


def test_table_lookups():
    """Every corpus n-gram is found by the restated probe with CiderD's own idf bits; absent n-grams end at an empty slot."""
    from vct_amd import rewards
    for name, refs, _ in _corpora():
        c = _cider(refs)
        T = c.device_tables()
        cap = T["table_cap"]
        assert cap & (cap - 1) == 0 and cap >= 2 * len(c.df) and T["table_keys"].shape == (cap, 4) and T["table_keys"].dtype == np.int32
        assert T["table_idf"].dtype == np.float64 and T["ent_w"].dtype == np.float64 and T["ref_norm"].dtype == np.float64
        assert int((T["table_keys"][:, 0] != -1).sum()) == len(c.df)
        worst = 0
        for w, df in c.df.items():
            found, idf, _, probes = D.probe(T, D.key_of(w))
            worst = max(worst, probes)
            assert found, (name, w)
            want = c.log_nvid - np.log(max(1, df))
            assert np.float64(idf).tobytes() == np.float64(c._vec({w: 1})[0][len(w) - 1][w]).tobytes(), (name, w)
            assert abs(idf - want) <= 1e-15 * max(abs(want), 1.0)
        print(f"[cider tables] {name}: {len(c.df)} n-grams in {cap} slots, longest probe {worst}")
        for w in [(1,), (3, 3, 3, 3), (999999, 5), (D.END, D.END), (0,)]:
            if w in c.df:
                continue
            found, idf, slot, _ = D.probe(T, D.key_of(w))
            assert not found and idf == c.log_nvid and T["table_keys"][slot, 0] == -1
        # the builder's vectorised hash is the header's
        keys = T["table_keys"][T["table_keys"][:, 0] != -1][:200]
        assert [int(h) for h in rewards.key_hash(keys)] == [D.key_hash(tuple(int(x) for x in k)) for k in keys]
        # the references' values are the host's own bits, sorted by key
        for vid, rs in c.refs.items():
            row = T["vid_row"][vid]
            r0, r1 = T["vid_ref_ptr"][row], T["vid_ref_ptr"][row + 1]
            assert r1 - r0 == len(rs)
            for r, (ln, vec, norm) in zip(range(r0, r1), rs):
                e0, e1 = T["ref_ent_ptr"][r], T["ref_ent_ptr"][r + 1]
                ks = [tuple(int(x) for x in k) for k in T["ent_keys"][e0:e1]]
                assert ks == sorted(ks) and len(set(ks)) == len(ks) == sum(len(d) for d in vec)
                assert T["ref_len"][r] == ln and T["ref_norm"][r, :c.n].tobytes() == np.asarray(norm, np.float64).tobytes()
                for k, v in zip(ks, T["ent_w"][e0:e1]):
                    w = tuple(t for t in k if t != -1)
                    assert np.float64(v).tobytes() == np.float64(vec[len(w) - 1][w]).tobytes()


@pytest.mark.parametrize("n,sigma", [(4, 6.0), (2, 0.5), (1, 6.0)])
def test_scoring_from_the_tables_alone(n, sigma):
    for name, refs, cands in _corpora():
        c = _cider(refs, n=n, sigma=sigma)
        T = c.device_tables()
        vids = list(refs)
        checked = 0
        for ids in cands:
            for b in range(ids.shape[0]):
                for s in range(ids.shape[1]):
                    cand = ids[b, s, 1:].tolist()
                    want = c.score(cand, vids[b])
                    got = D.score(T, cand, vids[b])
                    assert abs(got - want) <= FP64_TOL * abs(want), (name, b, s, got, want)
                    if want == 0.0:
                        assert got == 0.0
                    # the definition itself (slow: every idf is a scan of the corpus) on a sample of the large corpus
                    # (scst_ref.cider_d has no value for a video without references: CiderD's 0 is checked above)
                    if refs[vids[b]] and (name != "large" or b % 8 == 0):
                        ref = R.cider_d(cand, vids[b], refs, n=n, sigma=sigma, end_id=D.END)
                        assert abs(got - ref) <= FP64_TOL * max(abs(ref), 1e-300), (name, b, s, got, ref)
                        checked += 1
        assert checked > 0
        if name == "one_video":
            assert all(c.score(ids[0, s, 1:].tolist(), "only") == 0.0 for s in range(2))


@pytest.mark.parametrize("n,sigma", [(1, 6.0), (2, 6.0), (4, 6.0), (1, 0.5), (2, 0.5), (4, 0.5)])
@pytest.mark.parametrize("L", D.SMALL_LENGTHS)
def test_small_corpus_cases_do_not_score_zero(L, n, sigma):
    """The condition the GPU test states on its inputs, checked here as well: at least half of the candidates of the videos that
    have references score > 0 on the host, in fp32."""
    refs = D.small_corpus()
    ids = D.small_candidates(refs, L)
    r = _cider(refs, n=n, sigma=sigma)(ids, list(refs))
    assert r.dtype == np.float32 and (r[0] == 0).all()
    assert int((r[1:] > 0).sum()) * 2 >= r[1:].size, r


def test_device_tables_refusals():
    with pytest.raises(ValueError, match="orders up to 4"):
        _cider(D.small_corpus(), n=5).device_tables()
    with pytest.raises(ValueError, match="token ids"):
        _cider({0: [[3, -4, D.END]], 1: [[5, D.END]]}).device_tables()
    T = _cider({"a": [], "b": []}).device_tables()                  # no reference anywhere: empty tables, every video scores 0
    assert T["ent_keys"].shape == (0, 4) and list(T["vid_ref_ptr"]) == [0, 0, 0] and D.score(T, [3, D.END], "b") == 0.0


# ---- the C-ABI boundary -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from vct_amd import _lib
    return _lib.load()


def _desc(p, **kw):
    from vct_amd import _lib
    d = _lib.CiderDesc()
    d.B, d.N, d.L, d.n = 2, 3, 8, 4
    d.stride_b, d.stride_n, d.stride_l, d.end_id = 27, 9, 1, D.END
    d.log_nvid, d.two_sigma_sq, d.n_videos, d.table_cap = 1.0, 72.0, 2, 16
    for f in ("ids", "vid_rows", "table_keys", "table_idf", "vid_ref_ptr", "ref_len", "ref_norm", "ref_ent_ptr", "ent_keys", "ent_w", "reward"):
        setattr(d, f, p)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_entry_points_refuse_before_any_launch(lib):
    """Dummy host pointers: every call below must return its code without a launch.  Each refusal is tried on a descriptor whose
    reward pointer is NULL as well (VCT_E_ARG, checked later), so a missing shape check shows as the wrong code."""
    ARG, SHAPE, ALIGN = -1, -2, -3
    raw = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(raw) + 15) & ~15
    assert lib.vct_cider_d(None, None) == ARG
    assert lib.vct_cider_d(_desc(p, reward=None), None) == ARG
    assert lib.vct_cider_d(_desc(p, ids=None), None) == ARG and lib.vct_cider_d(_desc(p, ent_w=None), None) == ARG
    assert lib.vct_cider_d(_desc(p, L=65, reward=None), None) == SHAPE             # a 65-token candidate
    assert lib.vct_cider_d(_desc(p, L=64, reward=None), None) == ARG
    assert lib.vct_cider_d(_desc(p, n=5, reward=None), None) == SHAPE and lib.vct_cider_d(_desc(p, n=0, reward=None), None) == SHAPE
    assert lib.vct_cider_d(_desc(p, B=0, reward=None), None) == SHAPE and lib.vct_cider_d(_desc(p, L=-1, reward=None), None) == SHAPE
    assert lib.vct_cider_d(_desc(p, table_cap=24, reward=None), None) == SHAPE     # not a power of two
    for f in ("table_idf", "ref_norm", "ent_w"):                                   # fp64 tables: 8-byte aligned
        assert lib.vct_cider_d(_desc(p, B=0, **{f: p + 4}), None) == SHAPE
        assert lib.vct_cider_d(_desc(p, reward=None, **{f: p + 4}), None) == ARG
    # (the remaining refusal needs every operand: ALIGN is the last check, and with it the call still launches nothing)
    for f in ("table_idf", "ref_norm", "ent_w"):
        assert lib.vct_cider_d(_desc(p, **{f: p + 4}), None) == ALIGN
    assert lib.vct_cider_d(_desc(p, table_keys=p + 8), None) == ALIGN
    # vct_scst_advantages
    assert lib.vct_scst_advantages(2, 3, None, None, None, None, None, None) == ARG
    assert lib.vct_scst_advantages(2, 3, p, None, p, p, None, None) == ARG
    assert lib.vct_scst_advantages(2, 1, p, None, p, p, p, None) == SHAPE          # leave-one-out needs two samples
    assert lib.vct_scst_advantages(0, 3, p, p, p, p, p, None) == SHAPE


def test_table_builder_limits_are_the_kernels():
    """rewards' own limits against the binding's (and those against the header: tests/test_abi_cpu.py)."""
    from vct_amd import _lib, rewards
    assert (rewards.DEVICE_MAX_LEN, rewards.KEY_WORDS) == (_lib.CIDER_MAX_LEN, _lib.CIDER_MAX_ORDER)


def test_binding_lists_the_new_entries():
    from vct_amd import _lib
    assert {"vct_cider_d", "vct_scst_advantages"} <= set(_lib.exported_symbols()) and _lib.ABI_VERSION == 16
