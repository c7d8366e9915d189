"""Generation controls without a device (decode.GenerationControls, decode.apply_controls_host, the vct_logit_controls entry
point's refusals): the numpy restatement (tests/gen_controls_ref.py) against Hugging Face's logits processors, the torch
restatement against the numpy one bit for bit, the validation, the packed control block, and seeded faults that the comparisons
must catch."""
import ctypes
import struct

import numpy as np
import pytest
import torch

import gen_controls_ref as R

END = 2


def _hist(rng, rows, t, alphabet=4):
    return rng.integers(0, alphabet, (rows, t)).astype(np.int64)


def _grid(rng, rows, V):
    return (rng.integers(-40, 40, (rows, V)) / 8.0).astype(np.float32)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# ---- the restatement against Hugging Face's processors --------------------------------------------------------------------------
def _hf(x, hist, n=0, min_length=0, banned=(), theta=1.0):
    lp = pytest.importorskip("transformers.generation.logits_process")
    ids, s = torch.from_numpy(hist), x.clone()
    if theta != 1.0:
        s = lp.RepetitionPenaltyLogitsProcessor(float(theta))(ids, s)
    if n >= 1:
        s = lp.NoRepeatNGramLogitsProcessor(n)(ids, s)
    s = lp.MinLengthLogitsProcessor(min_length + 1, END)(ids, s)      # theirs counts the start token
    if banned:
        s = lp.NoBadWordsLogitsProcessor([[int(b)] for b in banned], eos_token_id=END)(ids, s)
    return s


def test_ngram_min_length_and_bans_equal_hugging_face():
    pytest.importorskip("transformers")
    rng = np.random.default_rng(0)
    V, rows = 9, 6
    for t in range(1, 65):
        hist = _hist(rng, rows, t)
        x = _grid(rng, rows, V)
        for n in range(1, 9):
            for m, banned in ((0, ()), (t, (5, 5, END)), (t - 1, (1,))):
                ours = R.apply(x, hist.tolist(), END, min_length=m, n=n, banned_ids=banned)
                theirs = _hf(torch.from_numpy(x), hist, n=n, min_length=m, banned=banned).numpy()
                assert np.array_equal(_bits(ours), _bits(theirs)), (t, n, m, banned)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_penalty_equals_hugging_face(dtype):
    """theta = 2 and 4: a division by a power of two is the multiplication by its reciprocal, exact.  theta = 1.3: theirs divides
    where ours multiplies by fp32(1 / theta): within one ulp of the dtype (the only tolerance here)."""
    pytest.importorskip("transformers")
    rng = np.random.default_rng(1)
    V, rows = 11, 8
    bf = dtype == torch.bfloat16
    for t in (1, 2, 5, 17, 64):
        hist = _hist(rng, rows, t)
        x = torch.from_numpy(_grid(rng, rows, V)).to(dtype)
        for theta in (2.0, 4.0, 1.3):
            ours = R.apply(x.float().numpy(), hist.tolist(), END, theta=theta, bf16=bf)
            theirs = _hf(x, hist, theta=theta).float().numpy()
            if theta != 1.3:
                assert np.array_equal(_bits(ours), _bits(theirs)), (t, theta)
            else:
                ulp = np.abs(theirs) * (2.0 ** -7 if bf else 2.0 ** -23)
                assert np.all(np.abs(ours - theirs) <= ulp), (t, theta)
    # all four together, exact at theta = 2
    hist = _hist(rng, rows, 20)
    x = torch.from_numpy(_grid(rng, rows, V))
    ours = R.apply(x.numpy(), hist.tolist(), END, min_length=25, n=3, theta=2.0, banned_ids=(7, 1))
    theirs = _hf(x, hist, n=3, min_length=25, banned=(7, 1), theta=2.0).numpy()
    assert np.array_equal(_bits(ours), _bits(theirs))


# ---- decode.apply_controls_host against the restatement, bit for bit ------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_apply_controls_host_equals_the_restatement(dtype):
    from vct_amd import decode
    rng = np.random.default_rng(2)
    V, ld, rows = 37, 40, 7
    bf = dtype == torch.bfloat16
    for t in (1, 2, 3, 7, 8, 30, 64):
        hist = _hist(rng, rows, t) + 1                       # tokens 1..4: END = 2 is in the history
        x = _grid(rng, rows, ld)
        x[:, V:] = 1e4
        xt = torch.from_numpy(x).to(dtype)
        ended = np.arange(rows) % 3 == 2
        for n in (0, 1, 2, 3, 8):
            for theta in (1.0, 1.5, 2.0, 1.3):
                for m, banned in ((0, ()), (t, (3, 3, END, 30))):
                    c = decode.GenerationControls(m, n, theta, banned)
                    got = decode.apply_controls_host(xt.clone(), torch.from_numpy(hist), END, c, torch.from_numpy(ended), V=V)
                    assert got.dtype == dtype
                    ref = R.apply(xt.float().numpy(), hist.tolist(), END, ended, bf, min_length=m, n=n, theta=theta, banned_ids=banned)
                    assert np.array_equal(_bits(got.float().numpy()), _bits(ref)), (t, n, theta, m)
                    assert np.array_equal(_bits(got.float().numpy()[ended]), _bits(xt.float().numpy()[ended]))
                    assert np.array_equal(_bits(got.float().numpy()[:, V:]), _bits(xt.float().numpy()[:, V:]))


# ---- the value object ------------------------------------------------------------------------------------------------------------
def test_validation_names_the_value():
    from vct_amd.decode import GenerationControls as G
    for kw, word in ((dict(min_length=-1), "min_length"), (dict(min_length=1.5), "min_length"),
                     (dict(no_repeat_ngram_size=9), "no_repeat_ngram_size"), (dict(no_repeat_ngram_size=-1), "no_repeat_ngram_size"),
                     (dict(repetition_penalty=0.99), "repetition_penalty"), (dict(repetition_penalty=16.5), "repetition_penalty"),
                     (dict(repetition_penalty=float("nan")), "repetition_penalty"), (dict(repetition_penalty=float("inf")), "repetition_penalty"),
                     (dict(banned_ids=range(33)), "banned_ids"), (dict(banned_ids=(-1,)), "banned_ids"), (dict(banned_ids=(1.5,)), "banned_ids")):
        with pytest.raises(ValueError, match=word):
            G(**kw)
    G(min_length=0, no_repeat_ngram_size=8, repetition_penalty=16, banned_ids=range(32))
    c = G(min_length=10, no_repeat_ngram_size=3, repetition_penalty=1.2, banned_ids=(5, 7))
    c.check(max_len=12, V=200)
    with pytest.raises(ValueError, match="min_length"):
        c.check(max_len=11, V=200)
    with pytest.raises(ValueError, match="max_len"):
        c.check(max_len=66, V=200)
    G(min_length=63).check(max_len=65, V=200)
    with pytest.raises(ValueError, match="banned_ids"):
        c.check(max_len=12, V=7)
    with pytest.raises(ValueError, match="at least one finite logit"):
        c.check(max_len=12, V=15)                            # V > 12 + 2 + 1 is needed
    c.check(max_len=12, V=16)
    with pytest.raises(AttributeError):
        c.min_length = 3
    assert c == G(10, 3, 1.2, [5, 7]) and hash(c) == hash(G(10, 3, 1.2, [5, 7])) and c != G(10, 3, 1.2, [5])


def test_is_noop():
    from vct_amd import decode
    G = decode.GenerationControls
    assert G().is_noop and G(0, 0, 1.0, ()).is_noop and G(banned_ids=[]).is_noop
    for c in (G(min_length=1), G(no_repeat_ngram_size=1), G(repetition_penalty=1.0001), G(banned_ids=(0,))):
        assert not c.is_noop
    assert decode._resolve_controls(None, 30, 1000) is None and decode._resolve_controls(G(), 30, 1000) is None
    assert decode._resolve_controls(G(), 500, 3) is None             # a no-op is not even checked
    c = G(min_length=2)
    assert decode._resolve_controls(c, 30, 1000) is c
    with pytest.raises(TypeError):
        decode._resolve_controls({"min_length": 2}, 30, 1000)


def test_packed_control_block():
    from vct_amd import _lib
    from vct_amd.decode import GenerationControls as G
    for kw in (dict(), dict(min_length=5, n=3, theta=1.2, banned_ids=(7, 7, 102)), dict(n=8, theta=16.0, banned_ids=tuple(range(100, 132)))):
        c = G(kw.get("min_length", 0), kw.get("n", 0), kw.get("theta", 1.0), kw.get("banned_ids", ()))
        raw = c.pack()
        assert len(raw) == 160 == ctypes.sizeof(_lib.LogitCtl)
        assert raw == R.pack(**kw)
        s = _lib.LogitCtl.from_buffer_copy(raw)
        assert (s.min_length, s.ngram, s.n_banned) == (c.min_length, c.no_repeat_ngram_size, len(c.banned_ids))
        assert list(s.banned)[:s.n_banned] == list(c.banned_ids) and list(s.reserved) == [0, 0, 0]
        assert struct.pack("<f", s.theta) == struct.pack("<f", c.repetition_penalty)
        assert struct.pack("<f", s.inv_theta) == struct.pack("<f", 1.0 / c.repetition_penalty)
        assert c.theta == s.theta and c.inv_theta == s.inv_theta


# ---- the entry point's refusals, through ctypes, without a device ---------------------------------------------------------------
def test_entry_point_refuses_before_any_launch():
    import __graft_entry__ as g
    g.build()
    from vct_amd import _lib
    lib = _lib.load()
    ARG, SHAPE = -1, -2
    raw = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(raw) + 15) & ~15

    def call(**kw):
        d = _lib.LogitControlsDesc()
        d.dtype, d.rows, d.V, d.t, d.x, d.ldx, d.end_id = _lib.BF16, 6, 70, 5, p, 72, 2
        d.ids, d.ids_stride, d.ended, d.ctl = p, 65, p, p
        for k, v in kw.items():
            setattr(d, k, v)
        return lib.vct_logit_controls(d, None)
    assert lib.vct_logit_controls(None, None) == ARG
    for name in ("x", "ids", "ended", "ctl"):
        assert call(**{name: None}) == ARG, name
        assert call(**{name: None}, t=0) == ARG, name                 # (argument errors come first)
    assert call(dtype=7, t=0) == ARG
    for kw in (dict(rows=0), dict(rows=-3), dict(V=0), dict(ldx=69), dict(t=0), dict(t=-1), dict(t=65)):
        assert call(**kw) == SHAPE, kw
    beams = dict(parents=p, parents_stride=6)
    for kw in (dict(K=0), dict(K=17), dict(K=-1), dict(K=4), dict(K=3, t=65), dict(K=3, t=0)):      # K = 4: 6 rows are no whole videos
        assert call(**beams, **kw) == SHAPE, kw
    assert call(K=17, t=65) == SHAPE and call(K=17, t=0) == SHAPE


# ---- seeded faults: what the bit-for-bit comparisons must be able to see ---------------------------------------------------------
def _fault_cases():
    rng = np.random.default_rng(3)
    for t in (2, 5, 9, 20):
        hist = _hist(rng, 5, t, alphabet=3) + 1
        x = _grid(rng, 5, 12)
        yield t, hist, x


def test_the_restatement_rejects_seeded_faults():
    seen = {"shift": 0, "twice": 0, "minlen": 0, "parents": 0}
    for t, hist, x in _fault_cases():
        good = R.apply(x, hist.tolist(), END, min_length=t, n=2, theta=1.5)
        # a ban shifted by one position: the token BEFORE the one the rule names
        def shifted(h, n):
            return {h[j - 1] for j in range(n - 1, len(h)) if h[j - n + 1:j] == h[len(h) - n + 1:]}
        if any(shifted(h, 2) != R.ngram_banned(h, 2) for h in hist.tolist()):
            seen["shift"] += 1
        # the penalty applied once per OCCURRENCE instead of once per distinct token
        twice = np.array(x, copy=True)
        for r, h in enumerate(hist.tolist()):
            for v in h:
                twice[r, v] = twice[r, v] / 1.5 if twice[r, v] > 0 else twice[r, v] * 1.5
        once = R.apply(x, hist.tolist(), END, theta=1.5)
        if any(len(set(h)) < len(h) for h in hist.tolist()):
            assert not np.array_equal(_bits(twice), _bits(once))
            seen["twice"] += 1
        # min_length off by one, both ways
        assert not np.array_equal(_bits(R.apply(x, hist.tolist(), END, min_length=t)), _bits(R.apply(x, hist.tolist(), END, min_length=t - 1)))
        assert np.array_equal(_bits(R.apply(x, hist.tolist(), END, min_length=t + 1)), _bits(R.apply(x, hist.tolist(), END, min_length=t)))
        assert np.all(R.apply(x, hist.tolist(), END, min_length=t)[:, END] == -np.inf)
        assert np.array_equal(R.apply(x, hist.tolist(), END, min_length=t - 1)[:, END], x[:, END])
        seen["minlen"] += 1
        assert good.shape == x.shape
    assert seen["shift"] >= 2 and seen["twice"] >= 3 and seen["minlen"] == 4
    # a beam history that ignores the parents: rows of the token table instead of the back-track
    rng = np.random.default_rng(4)
    K, B, Lmax, t, V = 3, 2, 12, 8, 12
    M = B * K
    tokens = rng.integers(1, 4, (M, Lmax)).astype(np.int64)
    tokens[:, 0] = 9
    parents = np.zeros((Lmax, M), np.int64)
    for s in range(1, Lmax):
        for b in range(B):
            parents[s, b * K:(b + 1) * K] = b * K + rng.permutation(K)
    x = _grid(rng, M, V)
    right = R.apply_beam(x, tokens, parents, t, END, n=2, theta=1.5)
    wrong = R.apply(x, tokens[:, :t].tolist(), END, n=2, theta=1.5)
    assert not np.array_equal(_bits(right), _bits(wrong))
    h = R.backtrack(tokens, parents, 4, t)
    r = 4
    for s in range(t - 1, 0, -1):
        assert h[s] == tokens[r, s] and parents[s, r] // K == 1
        r = parents[s, r]
    assert h[0] == 9 and len(h) == t


def test_ngram_rule_by_hand():
    """a b a b | a: with n = 2 the next token may not be b (a b exists); with n = 3 after a b a b the bigram (a, b) was followed by a."""
    a, b, c = 1, 2, 3
    assert R.ngram_banned([a, b, a], 2) == {b}
    assert R.ngram_banned([a, b, a, b], 3) == {a}
    assert R.ngram_banned([a, b, c], 1) == {a, b, c}
    assert R.ngram_banned([a], 3) == set() and R.ngram_banned([a, a], 3) == set() and R.ngram_banned([a, a, a], 3) == {a} and R.ngram_banned([a, b], 3) == set()
    assert R.ngram_banned([a, b, a], 0) == set()
