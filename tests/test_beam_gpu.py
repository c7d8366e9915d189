"""Beam search on the KV-cached decode path (csrc/vct_beam.hip, engine.BeamDecodeState, decode.beam_decode_ids):
the two kernels against numpy, the whole search against the numpy restatement (tests/beam_ref.py), K = 1 against greedy,
execution modes against each other, and the returned scores against a teacher-forced recomputation."""
import numpy as np
import pytest
import torch

import beam_ref
import vct_oracle as O
from helpers import build_model, load_golden, model_config_of

pytestmark = pytest.mark.gpu
DEV = "cuda"
END, PAD = 102, 0


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


# ---- vct_beam_select against numpy -----------------------------------------------------------------------------------------
def _select_inputs(B, K, V, seed):
    """Logits on a 1/8 grid (exact in bf16, many exact ties inside a row, one planted at the top of every row), video 0 at
    the first step (slot 0 scores 0, the others -inf), video 1 with finished slots, the rest unfinished.  Seeds are skipped
    until every near-tie between candidates of DIFFERENT rows in each video's top K + 1 is above 1e-3."""
    for s in range(seed, seed + 100):
        rng = np.random.default_rng(s)
        M = B * K
        x = (rng.integers(-80, 80, (M, V)) / 8.0).astype(np.float32)
        for r in range(M):
            c = int(x[r].argmax())
            x[r, (c + 1 + int(rng.integers(V - 1))) % V] = x[r, c]
        scores = (rng.normal(size=M) * 2.0 - 5.0).astype(np.float32)
        scores[:K] = -np.inf
        scores[0] = 0.0
        fin = np.zeros(M, bool)
        if B > 1:
            fin[K:2 * K] = rng.random(K) < 0.5
        if _cross_row_gaps_ok(x, scores, fin, K):
            return x, scores, fin
    raise AssertionError("no well-separated input found")


def _cross_row_gaps_ok(x, scores, fin, K):
    M, V = x.shape
    m = x.max(1, keepdims=True).astype(np.float64)
    lse = (m[:, 0] + np.log(np.exp(x - m).sum(1))).astype(np.float32)
    vals = (scores[:, None] + (x - lse[:, None])).astype(np.float64)
    vals[fin] = -np.inf
    vals[fin, PAD] = scores[fin]
    for b in range(M // K):
        v = vals[b * K:(b + 1) * K].reshape(-1)
        top = np.argsort(-v, kind="stable")[:K + 1]
        for a, c in zip(top[:-1], top[1:]):
            if a // V != c // V and np.isfinite(v[c]) and abs(v[a] - v[c]) < 1e-3:
                return False
    return True


def _run_select(x_np, scores, fin, K, dtype, ldx, t=5, Lmax=8):
    from vct_amd import ops
    M, V = x_np.shape
    B = M // K
    xs = torch.zeros(M, ldx, dtype=dtype, device=DEV)
    xs[:, :V] = torch.from_numpy(x_np).to(DEV, dtype)
    xs[:, V:] = 1e4                                      # columns past V must never be read as candidates
    sc = torch.from_numpy(scores).to(DEV)
    fn = torch.from_numpy(fin.astype(np.uint8)).to(DEV)
    parent = torch.full((M,), -7, dtype=torch.int32, device=DEV)
    ys = torch.full((M, Lmax), -5, dtype=torch.long, device=DEV)
    cnt = torch.zeros(1, dtype=torch.int32, device=DEV)
    at = torch.full((1,), Lmax, dtype=torch.long, device=DEV)
    ws = torch.empty(ops.beam_select_workspace_bytes(dtype, B, K, V) // 4, dtype=torch.float32, device=DEV)
    ops.beam_select(xs, B, K, sc, fn, parent, ys[:, t], END, PAD, cnt, at, t, ws, cols=V)
    torch.cuda.synchronize()
    assert torch.all(ys[:, :t] == -5) and torch.all(ys[:, t + 1:] == -5)
    return (parent.cpu().numpy(), ys[:, t].cpu().numpy(), sc.cpu().numpy(), fn.cpu().numpy().astype(bool), int(cnt[0]), int(at[0]))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("K", [1, 2, 4, 5, 8, 16])
@pytest.mark.parametrize("V", [257, 30522])
def test_beam_select_matches_numpy(V, K, dtype):
    B = 3
    for ldx in ((V + 31) // 32 * 32 + 32, V + 3):        # 16-byte rows (vector loads) and odd rows (element loads), both > V
        x, scores, fin = _select_inputs(B, K, V, seed=17 * K + V)
        xq = torch.from_numpy(x).to(dtype).float().numpy()
        parent, tok, ns, nf, cnt, at = _run_select(x, scores, fin, K, dtype, ldx)
        rp, rt, rs, rf, _ = beam_ref.select_step(xq, scores, fin, K, PAD, END)
        assert np.array_equal(parent, rp), (ldx, parent, rp)
        assert np.array_equal(tok, rt), (ldx, tok, rt)
        assert np.array_equal(nf, rf)
        np.testing.assert_allclose(ns, rs, rtol=1e-6, atol=0)
        assert cnt == int(rf.sum()) and at == (5 if rf.all() else 8)


def test_beam_select_all_finished_records_the_step():
    """Every slot finished after the step -> all_finished_at = t; the frozen slots come out in score order with pad tokens."""
    K, V = 3, 257
    rng = np.random.default_rng(3)
    x = rng.normal(size=(2 * K, V)).astype(np.float32)
    scores = np.array([-1.0, -3.0, -2.0, -4.0, -0.5, -6.0], np.float32)
    fin = np.ones(2 * K, bool)
    parent, tok, ns, nf, cnt, at = _run_select(x, scores, fin, K, torch.float32, V)
    assert parent.tolist() == [0, 2, 1, 4, 3, 5] and np.all(tok == PAD) and nf.all()
    assert ns.tolist() == [-1.0, -2.0, -3.0, -0.5, -4.0, -6.0]
    assert cnt == 2 * K and at == 5


# ---- vct_beam_reorder against index_select ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,d", [(torch.bfloat16, 64), (torch.float32, 64), (torch.bfloat16, 20), (torch.float32, 18)])
def test_beam_reorder_matches_index_select(dtype, d):
    from vct_amd import ops
    L, B, K, Lmax = 3, 5, 4, 30
    M = B * K
    g = torch.Generator(device="cpu").manual_seed(1)
    for t in (1, 17, Lmax - 1):
        src = torch.randn(L, M * Lmax, 3 * d, generator=g).to(DEV, dtype)
        dst = torch.randn(L, M * Lmax, 3 * d, generator=g).to(DEV, dtype)
        parent = (torch.arange(B)[:, None] * K + torch.randint(0, K, (B, K), generator=g)).reshape(M).to(DEV, torch.int32)
        want = dst.clone().view(L, M, Lmax, 3 * d)
        want[:, :, :t, d:] = src.view(L, M, Lmax, 3 * d).index_select(1, parent.long())[:, :, :t, d:]
        ops.beam_reorder(src, dst, parent, M, Lmax, d, t)
        torch.cuda.synchronize()
        assert torch.equal(dst.view(L, M, Lmax, 3 * d), want), t


# ---- end to end against the numpy reference (fp32) -------------------------------------------------------------------------
def _tiny():
    z = load_golden("tiny_decode.npz")
    mc, V = model_config_of(z), int(z["vocab"])
    cfg = O.cfg_from_model_config(mc, V)
    p = O.init_params(cfg, seed=int(z["param_seed"]))
    return z, mc, V, cfg, p


def _check_vs_numpy(m, p, cfg, feats_np, K, max_len):
    from vct_amd import decode
    ids_ref, fin_ref, margin = beam_ref.beam_search(p, cfg, feats_np, None, K, max_len=max_len)
    assert margin > 1e-4, margin                  # no unresolvable near-tie on the way
    feats = torch.from_numpy(feats_np).to(DEV)
    ids, fin = decode.beam_decode_ids(m, feats, None, K, max_len=max_len, return_all=True)
    assert np.array_equal(ids.cpu().numpy(), ids_ref)
    np.testing.assert_allclose(fin.cpu().numpy(), fin_ref, rtol=1e-4)
    best = m.beam_decode_ids([feats], None, beam_size=K, max_len=max_len)
    assert np.array_equal(best.cpu().numpy(), ids_ref[:, 0])
    # the reference algorithm (full decoder re-run per token, host-side selection) follows the same semantics
    (ids_alg, fin_alg), margin_alg = decode.beam_decode_ids_reference_algorithm(m, feats, None, K, max_len=max_len, return_all=True)
    assert margin_alg > 1e-4 and np.array_equal(ids_alg.cpu().numpy(), ids_ref)
    np.testing.assert_allclose(fin_alg.cpu().numpy(), fin_ref, rtol=1e-4)


def test_tiny_fp32_beam_matches_numpy():
    z, mc, V, cfg, p = _tiny()
    m = build_model(mc, V, DEV, torch.float32, p)
    for tag in ("b1", "b3"):
        _check_vs_numpy(m, p, cfg, z[f"{tag}/feats"], 3, 12)


def test_step_tail_of_every_session_kind(monkeypatch):
    """The tail of a decode step, per kind of session: generation controls (only where the session carries them) in front of the
    session's own selection stage, beams alone hand their parent rows to the controls, and every beam step reorders the cache from
    the ping-pong side it ran on into the other.  Eager decodes of three steps; only the names of the ops wrappers are looked at."""
    from vct_amd import decode, ops
    z, mc, V, cfg, p = _tiny()
    m = build_model(mc, V, DEV, torch.float32, p)
    feats = torch.from_numpy(z["b3/feats"]).to(DEV)
    calls = []

    def wrap(name):
        real = getattr(ops, name)

        def wrapped(*a, **k):
            calls.append((name, a, k))
            return real(*a, **k)
        monkeypatch.setattr(ops, name, wrapped)
    for name in ("greedy_select", "logit_controls", "beam_select", "beam_reorder", "sample_select"):
        wrap(name)
    ctl = decode.GenerationControls(min_length=1, no_repeat_ngram_size=2)
    kw = dict(max_len=4, use_graphs=False)
    decoders = {"greedy": (lambda c: decode.greedy_decode_ids(m, feats, None, controls=c, **kw), ["greedy_select"]),
                "beam": (lambda c: decode.beam_decode_ids(m, feats, None, 2, controls=c, **kw), ["beam_select", "beam_reorder"]),
                "sample": (lambda c: decode.sample_decode_ids(m, feats, None, num_samples=2, top_k=1, controls=c, **kw),
                           ["sample_select"])}
    for kind, (run, stage) in decoders.items():
        for c in (None, ctl):
            del calls[:]
            m.__dict__.pop("_decode_sessions", None)          # the run's session is then the only one cached
            run(c)
            assert [n for n, _, _ in calls] == (([] if c is None else ["logit_controls"]) + stage) * 3, (kind, c)
            for n, a, k in calls:
                if n == "logit_controls":
                    if kind == "beam":
                        assert k["K"] == 2 and k["parents"] is not None
                    else:
                        assert k.get("parents") is None and not k.get("K") and len(a) == 6
            if kind == "beam":
                ((key, st),) = m.__dict__["_decode_sessions"].items()
                assert key[0] == "beam" and ("ctl" in key) == (c is not None)
                reorders = [a for n, a, _ in calls if n == "beam_reorder"]
                for t, a in enumerate(reorders, start=1):
                    assert a[0].data_ptr() == st.kv_layers[t % 2].data_ptr(), t
                    assert a[1].data_ptr() == st.kv_layers[(t + 1) % 2].data_ptr(), t
                assert st.kv_layers[0].data_ptr() != st.kv_layers[1].data_ptr()


@pytest.mark.parametrize("K", [2, 4])
def test_cfgA_fp32_beam_matches_numpy(K):
    z = load_golden("cfgA_decode.npz")
    mc = model_config_of(load_golden("cfgA_slices.npz"))
    cfg = O.cfg_from_model_config(mc, 30522)
    p = O.init_params(cfg, seed=int(z["param_seed"]))
    f = O.synthetic_batch(4, 12, 512, 20, 30522, seed=int(z["feats_seed"]))[0]
    m = build_model(mc, 30522, DEV, torch.float32, p)
    _check_vs_numpy(m, p, cfg, f, K, 30)


# ---- cfg-B: K = 1 vs greedy, execution modes, teacher-forced scores ---------------------------------------------------------
@pytest.fixture(scope="module")
def cfgB():
    z = load_golden("cfgB_decode.npz")
    mc, V = model_config_of(z), int(z["vocab"])
    cfg = O.cfg_from_model_config(mc, V)
    p = O.init_params(cfg, seed=int(z["param_seed"]))
    return z, mc, V, p, {}


def _cfgB_model(cfgB, dtype):
    z, mc, V, p, cache = cfgB
    if dtype not in cache:
        cache[dtype] = build_model(mc, V, DEV, dtype, p)
    return cache[dtype]


def _cfgB_feats(B, seed=5):
    return torch.from_numpy(O.synthetic_batch(B, 12, 512, 20, 30522, seed=seed)[0]).to(DEV)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("B", [1, 3, 16])
def test_beam_k1_is_greedy(cfgB, dtype, B, monkeypatch):
    from vct_amd import engine
    if B == 1:      # greedy's batch-1 block step is greedy-only: both decodes on the gemv step, as beams at B*K = 1
        monkeypatch.setattr(engine.DecoderEngine, "block_decode", False)
    m = _cfgB_model(cfgB, dtype)
    feats = _cfgB_feats(B, seed=40 + B)
    g = m.greedy_decode_ids([feats], None, max_len=30).cpu().numpy()
    b1 = m.beam_decode_ids([feats], None, beam_size=1, max_len=30).cpu().numpy()
    assert b1.shape == g.shape
    for r in range(B):
        hits = np.flatnonzero(g[r] == END)
        n = hits[0] + 1 if hits.size else g.shape[1]
        assert np.array_equal(b1[r, :n], g[r, :n]), r
        assert np.all(b1[r, n:] == PAD)


def test_bf16_execution_modes_agree_and_scores_follow_the_cache(cfgB):
    from vct_amd import decode, engine
    m = _cfgB_model(cfgB, torch.bfloat16)
    dec = m.cap_decoder._engine()
    B, K = 16, 4
    feats = _cfgB_feats(B)
    st = engine.BeamDecodeState(dec, B, K, 13, 30)
    assert engine._decoder_fused_decode_ok(dec, st)          # the path under test is the fused bf16 step
    run = lambda **kw: decode.beam_decode_ids(m, feats, None, K, max_len=30, return_all=True, **kw)
    ids, fin = run()
    for other in (run(), run(use_graphs=False)):
        assert torch.equal(ids, other[0]) and torch.equal(fin, other[1])
    # other sessions and a greedy decode in between leave the result alone
    decode.beam_decode_ids(m, _cfgB_feats(3, seed=9), None, 2, max_len=30)
    m.greedy_decode_ids([feats], None, max_len=30)
    decode.beam_decode_ids(m, feats, None, 3, max_len=30)
    again = run()
    assert torch.equal(ids, again[0]) and torch.equal(fin, again[1])
    # the reference algorithm (full decoder per token, host selection) where its margins are resolvable in bf16
    checked = 0
    for b in range(B):
        ref, margin = decode.beam_decode_ids_reference_algorithm(m, feats[b:b + 1], None, K, max_len=30, return_all=True)
        if margin > 0.15:                                    # bf16 cannot resolve smaller gaps between two kernel paths
            n = min(ref[0].shape[2], ids.shape[2])
            assert torch.equal(ref[0][0, :, :n], ids[b, :, :n]), b
            checked += 1
    print(f"reference algorithm compared on {checked} of {B} videos")
    # every hypothesis's score, recomputed along its own ids with the greedy KV-cache step (teacher forced)
    Lp = ids.shape[2]
    flat = ids.reshape(B * K, Lp)
    _, lg = decode.teacher_forced_next_ids(m, feats.repeat_interleave(K, 0), None, flat, Lp - 1, return_logits=True)
    logp = torch.log_softmax(lg.double(), dim=2)
    gen = flat[:, 1:] == END
    n = torch.where(gen.any(1), gen.int().argmax(1) + 1, torch.full_like(gen[:, 0], Lp - 1, dtype=torch.long))
    tok_lp = logp.gather(2, flat[:, 1:, None])[:, :, 0]
    keep = torch.arange(Lp - 1, device=DEV)[None, :] < n[:, None]
    want = (tok_lp * keep).sum(1)
    raw = fin.reshape(-1).double() * n.double()
    assert torch.all((raw - want).abs() <= 2e-2 * want.abs()), (raw - want).abs().max()


def test_module_api_and_stop_rule():
    from vct_amd import evaluate
    z, mc, V, cfg, p = _tiny()
    m = build_model(mc, V, DEV, torch.float32, p)
    feats = torch.from_numpy(z["b3/feats"]).to(DEV)
    caps = m.beam_decode([feats], None, beam_size=3, max_len=12)
    assert isinstance(caps, list) and len(caps) == 3 and all(isinstance(c, str) for c in caps)
    assert len(evaluate.v2t_batch(m, [feats], None, max_len=12, beam_size=3)) == 3
    assert isinstance(evaluate.v2t_single(m, [feats[0]], max_len=12, beam_size=2), str)
    for max_len in (5, 12, 30):
        ids = m.beam_decode_ids([feats], None, beam_size=3, max_len=max_len)
        st = m._decode_sessions[("beam", 3, 3, feats.shape[1] + 1, max_len, torch.float32)]
        at = int(st.all_ended_at[0])
        assert ids.shape[1] == min(at, max_len - 1) + 1 and ids.shape[1] <= max_len
    with pytest.raises(ValueError):
        m.beam_decode_ids([feats], None, beam_size=17)
