"""decode.Ensemble end to end on the device: exact identities against smaller ensembles, every generated token / beam score /
sampled log-probability against an fp64 recombination of the members' own teacher-forced logits (tests/ensemble_ref.py), controls,
graphs against eager launches, mixed dtypes and encoder types, and the evaluate entry points.

Tiny models (ensemble_ref.tiny_models): A d 64 / ff 128 / 2 + 2 layers, B another seed, d 32 / ff 64 / 1 + 3 layers, V 131, fp32
compute unless stated."""
import pytest
import torch

import ensemble_ref as ER

pytestmark = pytest.mark.gpu
DEV = "cuda"
START, END, PAD = 101, 102, 0
V = ER.V_TINY
MAX_LEN = 10
F64 = torch.float64


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@pytest.fixture(scope="module")
def ab():
    return ER.tiny_models(DEV)


def _graphs(ens):
    return sum(len(st.graphs) + (st.begin is not None) for st in ens.__dict__["_decode_sessions"].values())


def _bits(t):
    return t.contiguous().view(torch.int32)


def _all_three(ens, feats, **kw):
    """Greedy ids, beam ids + scores (K = 3, return_all), sampled ids + seq_logp (two samples per video, seed 11)."""
    g = ens.greedy_decode_ids(feats, None, MAX_LEN, **kw)
    bi, bs = ens.beam_decode_ids(feats, None, 3, MAX_LEN, return_all=True, **kw)
    si, sl = ens.sample_decode_ids(feats, None, MAX_LEN, 2, seed=11, return_logp=True, **kw)
    return g, bi, bs, si, sl


def _same(a, b):
    ga, bia, bsa, sia, sla = a
    gb, bib, bsb, sib, slb = b
    assert torch.equal(ga, gb), "greedy ids"
    assert torch.equal(bia, bib) and torch.equal(_bits(bsa), _bits(bsb)), "beam ids / scores"
    assert torch.equal(sia, sib) and torch.equal(_bits(sla), _bits(slb)), "sampled ids / seq_logp"


# ---- exact identities -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
def test_a_twice_in_logprob_mode_is_a(ab, B):
    from vct_amd import decode
    a, _ = ab
    feats = ER.tiny_batch(B, 3, DEV)
    _same(_all_three(decode.Ensemble([a, a], mode="logprob"), feats), _all_three(decode.Ensemble([a], mode="logprob"), feats))


@pytest.mark.parametrize("B", [1, 3])
def test_unit_weights_select_one_member_without_recapture(ab, B):
    from vct_amd import decode
    a, b = ab
    feats = ER.tiny_batch(B, 4, DEV)
    pair = decode.Ensemble([a, b], weights=[1, 0])
    first = _all_three(pair, feats)
    _same(first, _all_three(decode.Ensemble([a]), feats))
    sessions, n = dict(pair.__dict__["_decode_sessions"]), _graphs(pair)
    assert len(sessions) == 3 and 6 <= n <= 3 * MAX_LEN        # three sessions: a begin graph and up to MAX_LEN - 1 step graphs each
    pair.set_weights([0, 1])
    second = _all_three(pair, feats)
    _same(second, _all_three(decode.Ensemble([b]), feats))
    assert _graphs(pair) == n and all(pair.__dict__["_decode_sessions"][k] is st for k, st in sessions.items())
    assert not torch.equal(_bits(first[2]), _bits(second[2]))           # (the two members do score differently)


@pytest.mark.parametrize("B", [1, 3])
def test_eager_launches_equal_the_graphs(ab, B):
    from vct_amd import decode
    a, b = ab
    feats = ER.tiny_batch(B, 5, DEV)
    ens = decode.Ensemble([a, b], weights=[2, 1])
    _same(_all_three(ens, feats), _all_three(ens, feats, use_graphs=False))


# ---- against the fp64 recombination of the members' teacher-forced logits ---------------------------------------------------------------------
def _member_logits(models, feats, ids, rep=1):
    """Every member's fp32 logits [rows * steps, V] along the id rows `ids` [rows, L] (rows = videos * rep), from the single-model
    teacher-forced decode step."""
    from vct_amd import decode
    f = [x.repeat_interleave(rep, 0) for x in feats]
    steps = ids.shape[1] - 1
    return [decode.teacher_forced_next_ids(m, f, None, ids, steps, return_logits=True)[1].reshape(-1, V) for m in models]


def _path_logp(models, w, mode, feats, ids, rep):
    """fp64 sum of the combined, renormalised log-probabilities along each id row up to and including its first END, and its bound.
    Per step the selection kernels form out[tok] - logsumexp(out) in fp32 from the combined row `out`: the combined row's own bound
    enters at the token and, through the logsumexp (whose derivative is the softmax p, summing to 1), as sum_v p_v bound_v; the
    selection's exp / log are granted E (1 + |lse|) like every device log here, its subtraction and the running sum u each."""
    rows, L = ids.shape
    out, bound = ER.combine(_member_logits(models, feats, ids, rep), w, mode)
    lse = torch.logsumexp(out, 1, keepdim=True)
    p = torch.exp(out - lse)
    tok = ids[:, 1:].reshape(-1, 1)
    lp = (out.gather(1, tok) - lse).view(rows, L - 1)
    e = (bound.gather(1, tok) + (p * bound).sum(1, keepdim=True) + ER.E * (1.0 + lse.abs())
         + 4 * ER.U24 * (out.gather(1, tok).abs() + lse.abs())).view(rows, L - 1)
    ended = torch.cumsum((ids[:, 1:] == END).long(), 1) - (ids[:, 1:] == END).long() > 0      # strictly after the first END
    lp, e = lp.masked_fill(ended, 0.0), e.masked_fill(ended, 0.0)
    total = lp.sum(1)
    return total, e.sum(1) + L * ER.U24 * lp.abs().sum(1)


@pytest.mark.parametrize("mode", ["prob", "logprob"])
@pytest.mark.parametrize("B", [1, 3])
def test_every_greedy_token_is_the_fp64_argmax(ab, B, mode):
    from vct_amd import decode
    a, b = ab
    feats = ER.tiny_batch(B, ER.GAP_SEED, DEV)
    w = [0.6, 0.4]
    ys = decode.Ensemble([a, b], weights=w, mode=mode).greedy_decode_ids(feats, None, MAX_LEN)
    assert ys.shape[0] == B and 2 <= ys.shape[1] <= MAX_LEN and bool((ys[:, 0] == START).all())
    out, bound = ER.combine(_member_logits([a, b], feats, ys), w, decode.ensemble.MODES[mode])
    top = out.topk(2, dim=1)
    gap = top.values[:, 0] - top.values[:, 1]
    need = bound.gather(1, top.indices).sum(1)
    print(f"[ensemble] greedy {mode} B {B}: smallest top-2 gap / bound = {float((gap / need).min()):.1f} over {gap.numel()} positions")
    assert bool((gap > need).all()), "the batch seed must keep every position's top-2 gap outside the bound (ensemble_ref.GAP_SEED)"
    assert torch.equal(ys[:, 1:].reshape(-1), top.indices[:, 0])


@pytest.mark.parametrize("mode", ["prob", "logprob"])
def test_beam_scores_are_fp64_path_sums(ab, mode):
    from vct_amd import decode
    a, b = ab
    B, K, w = 3, 3, [0.6, 0.4]
    feats = ER.tiny_batch(B, 6, DEV)
    ens = decode.Ensemble([a, b], weights=w, mode=mode)
    ids, scores = ens.beam_decode_ids(feats, None, K, MAX_LEN, length_penalty=0.0, return_all=True)
    assert ids.shape[:2] == (B, K) and scores.shape == (B, K)
    assert bool((scores[:, :-1] >= scores[:, 1:]).all()), "beams sorted best first"
    want, bound = _path_logp([a, b], w, decode.ensemble.MODES[mode], feats, ids.reshape(B * K, -1), K)
    ER.check(f"beam scores {mode}", scores.reshape(-1), want, bound)
    best = ens.beam_decode_ids(feats, None, K, MAX_LEN, length_penalty=0.0)
    assert torch.equal(best, ids[:, 0])


@pytest.mark.parametrize("mode", ["prob", "logprob"])
def test_sampling(ab, mode):
    from vct_amd import decode
    a, b = ab
    B, N, w = 3, 2, [0.6, 0.4]
    feats = ER.tiny_batch(B, 7, DEV)
    ens = decode.Ensemble([a, b], weights=w, mode=mode)
    greedy = ens.greedy_decode_ids(feats, None, MAX_LEN)
    top1 = ens.sample_decode_ids(feats, None, MAX_LEN, 1, top_k=1, seed=5)
    for r in range(B):                                        # greedy up to and including each row's first END
        g, s = greedy[r].tolist(), top1[r, 0].tolist()
        n = min((g.index(END) + 1) if END in g else len(g), len(s))
        assert g[:n] == s[:n] and all(t == PAD for t in s[n:])
    ids, lp = ens.sample_decode_ids(feats, None, MAX_LEN, N, temperature=1.0, seed=21, return_logp=True)
    want, bound = _path_logp([a, b], w, decode.ensemble.MODES[mode], feats, ids.reshape(B * N, -1), N)
    ER.check(f"sampled seq_logp {mode}", lp.reshape(-1), want, bound)
    ids2, lp2 = ens.sample_decode_ids(feats, None, MAX_LEN, N, temperature=1.0, seed=21, return_logp=True)
    assert torch.equal(ids, ids2) and torch.equal(_bits(lp), _bits(lp2)), "a seed reproduces bit for bit"
    assert ens.sample_decode_ids(feats, None, MAX_LEN, N, temperature=1.0, seed=22).shape[:2] == (B, N)


# ---- controls, mixed members, the evaluate entry points ---------------------------------------------------------------------------------------
def test_controls_act_on_the_combined_distribution(ab):
    from vct_amd import decode
    a, b = ab
    feats = ER.tiny_batch(3, 8, DEV)
    ens = decode.Ensemble([a, b])
    plain = ens.greedy_decode_ids(feats, None, MAX_LEN)
    banned, min_length = int(plain[0, 1]), 6
    c = decode.GenerationControls(min_length, 0, 1.0, (banned,))
    ys = ens.greedy_decode_ids(feats, None, MAX_LEN, controls=c)
    assert int(ys[0, 1]) != banned and ys.shape[1] > min_length
    for row in ys.tolist():
        assert banned not in row[1:] and (END not in row or row.index(END) > min_length)
    ids, _ = ens.beam_decode_ids(feats, None, 3, MAX_LEN, return_all=True, controls=c)
    for row in ids.reshape(-1, ids.shape[-1]).tolist():
        cut = row[:row.index(END) + 1] if END in row else row
        assert banned not in cut[1:] and (END not in row or row.index(END) > min_length)
    s = ens.sample_decode_ids(feats, None, MAX_LEN, 2, seed=3, controls=c)
    for row in s.reshape(-1, s.shape[-1]).tolist():
        cut = row[:row.index(END) + 1] if END in row else row
        assert banned not in cut[1:] and (END not in row or row.index(END) > min_length)
    assert torch.equal(ens.greedy_decode_ids(feats, None, MAX_LEN), plain)       # the session without controls is untouched


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("pair", ["fp32+bf16", "mme+hmme"])
def test_mixed_members_decode(pair, B):
    from vct_amd import decode
    a, b = ER.tiny_models(DEV, dtype_a=torch.bfloat16) if pair == "fp32+bf16" else ER.tiny_models(DEV, hmme_b=True)
    feats = ER.tiny_batch(B, 9, DEV)
    ens = decode.Ensemble([b, a])
    for mode_out in (ens.greedy_decode_ids(feats, None, MAX_LEN), ens.beam_decode_ids(feats, None, 3, MAX_LEN),
                     ens.sample_decode_ids(feats, None, MAX_LEN, 1, seed=1)[:, 0]):
        assert mode_out.shape[0] == B and 2 <= mode_out.shape[1] <= MAX_LEN and mode_out.dtype == torch.int64
        assert bool(((mode_out >= 0) & (mode_out < V)).all()) and bool((mode_out[:, 0] == START).all())
    _, scores = ens.beam_decode_ids(feats, None, 3, MAX_LEN, return_all=True)
    _, lp = ens.sample_decode_ids(feats, None, MAX_LEN, 2, seed=1, return_logp=True)
    assert bool(torch.isfinite(scores).all()) and bool(torch.isfinite(lp).all())


def test_evaluate_takes_an_ensemble(ab):
    from vct_amd import decode, evaluate
    a, b = ab
    B = 3
    feats = [f.cpu() for f in ER.tiny_batch(B, 10, DEV)]
    ens = decode.Ensemble([a, b])
    for kw in (dict(), dict(beam_size=3)):
        caps = evaluate.v2t_batch(ens, feats, None, max_len=MAX_LEN, **kw)
        assert len(caps) == B and all(isinstance(c, str) for c in caps)
    sampled = evaluate.v2t_batch(ens, feats, None, max_len=MAX_LEN, sample=dict(num_samples=2, seed=4))
    assert len(sampled) == B and all(len(c) == 2 and all(isinstance(s, str) for s in c) for c in sampled)
    one = evaluate.v2t_single(ens, [f[0] for f in feats], max_len=MAX_LEN)
    assert isinstance(one, str)
    dev_feats = ER.tiny_batch(B, 10, DEV)
    assert ens.greedy_decode(dev_feats, None, MAX_LEN) == a._ids_to_captions(ens.greedy_decode_ids(dev_feats, None, MAX_LEN))
    with pytest.raises(ValueError, match="return_attn"):
        evaluate.v2t_batch(ens, feats, None, max_len=MAX_LEN, return_attn=True)
    with pytest.raises(ValueError, match="return_attn"):
        ens.greedy_decode_ids(ER.tiny_batch(B, 10, DEV), None, MAX_LEN, return_attn=True)
