"""Sampled decoding on the KV-cached decode path (csrc/vct_sample.hip, engine.SampleDecodeState, decode.sample_decode_ids): the
selection kernel through the C ABI against the numpy restatement (tests/sample_ref.py), its distribution, its sticky state over
launches, and the whole decode against greedy, against itself in other execution modes, against the reference algorithm and
against a teacher-forced recomputation."""
import functools

import numpy as np
import pytest
import torch

import sample_ref as S
import vct_oracle as O
from helpers import build_model, load_golden, model_config_of

pytestmark = pytest.mark.gpu
DEV = "cuda"
END, PAD = 102, 0
# ten times the bound for the fp32 error of a tree-ordered sum of up to 30522 expf terms (about 15 levels x 6e-8 plus expf's 2 ulp)
DELTA = 1e-5


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


# ---- vct_sample_select against the restatement ---------------------------------------------------------------------------------
def _ctl(seed, top_k, temperature, top_p):
    c = np.zeros(1, dtype=[("seed", "<u4"), ("k", "<i4"), ("it", "<f4"), ("p", "<f4")])
    c["seed"], c["k"], c["it"], c["p"] = seed, top_k, np.float32(1.0 / temperature), np.float32(top_p)
    return torch.from_numpy(c.view(np.int32).copy()).to(DEV)


@functools.lru_cache(maxsize=None)
def _case(V, rows, top_k, top_p, temperature, t=5):
    """Logits on a 1/8 grid (exact in bf16, many exact ties, one planted at the top of every row), a third of the rows already
    ended, and the restatement's answer.  Generator seeds are skipped until the restatement alone keeps the rows within DELTA of
    a boundary at or below 1 % and every nucleus cut more than DELTA away from a running share."""
    end = 0 if V == 1 else 3
    for s in range(1000 * V + 10 * rows + top_k, 1000 * V + 10 * rows + top_k + 50):
        rng = np.random.default_rng(s)
        x = (rng.integers(-80, 80, (rows, V)) / 8.0).astype(np.float32)
        if V > 1:
            for r in range(rows):
                c = int(x[r].argmax())
                x[r, (c + 1 + int(rng.integers(V - 1))) % V] = x[r, c]
        if top_k == 0 and V > 1000:
            # Over the whole of a large vocabulary most tokens' shares of [0, 1) are narrower than 2 * DELTA, and a draw that
            # lands on one is undecided by definition: the 1 % cap needs the mass in wide shares.  Eight planted columns per
            # row (an exact tie at the top, offsets in units of the temperature, still on the grid and exact in bf16) take all
            # but ~0.3 % of it; the 30514 others keep enough for an error in their sum to show in step_logp.
            base = {0.5: 16.125, 1.0: 22.375, 2.0: 35.0}[temperature]
            for r in range(rows):
                cols = rng.choice(V, 8, replace=False)
                x[r, cols] = base - temperature * np.array([0, 0, 1, 2, 2, 3, 5, 8], np.float32)
        ended = np.arange(rows) % 3 == 1
        seed = int(rng.integers(0, 2 ** 32))
        ref = S.select_step(x, ended, seed, t, np.float32(1.0 / temperature), top_k, top_p, PAD, end)
        if (ref[3] <= DELTA).mean() <= 0.01 and np.all(ref[4] > DELTA):
            return x, ended, seed, end, ref
    raise AssertionError("no input within the caps found")


def _run_select(x_np, ended, dtype, ldx, ctl, end, t=5, Lmax=8, seq0=None):
    """One call through ops.sample_select (the ctypes descriptor of the C ABI) with canaries around out, step_logp and seq_logp."""
    from vct_amd import ops
    rows, V = x_np.shape
    xs = torch.zeros(rows, ldx, dtype=dtype, device=DEV)
    xs[:, :V] = torch.from_numpy(x_np).to(DEV, dtype)
    xs[:, V:] = 1e4                                      # columns past V must never be read as candidates
    ys = torch.full((rows + 2, Lmax), -5, dtype=torch.long, device=DEV)
    lp = torch.full((rows + 16,), 77.0, dtype=torch.float32, device=DEV)
    sq = torch.full((rows + 16,), 55.0, dtype=torch.float32, device=DEV)
    seq0 = np.linspace(-3.0, 2.0, rows).astype(np.float32) if seq0 is None else seq0
    sq[8:8 + rows] = torch.from_numpy(seq0).to(DEV)
    en = torch.from_numpy(ended.astype(np.uint8)).to(DEV)
    cnt = torch.full((1,), int(ended.sum()), dtype=torch.int32, device=DEV)
    at = torch.full((1,), Lmax, dtype=torch.long, device=DEV)
    ws = torch.full((ops.sample_select_workspace_bytes(dtype, rows, V) // 4,), float("nan"), dtype=torch.float32, device=DEV)
    ops.sample_select(xs, ys[1:1 + rows, t], end, PAD, en, cnt, at, t, lp[8:8 + rows], sq[8:8 + rows], ctl, ws, cols=V)
    torch.cuda.synchronize()
    ysc = ys.cpu().numpy()
    keep = np.ones_like(ysc, bool)
    keep[1:1 + rows, t] = False
    assert np.all(ysc[keep] == -5)
    lpc, sqc = lp.cpu().numpy(), sq.cpu().numpy()
    assert np.all(lpc[:8] == 77.0) and np.all(lpc[8 + rows:] == 77.0) and np.all(sqc[:8] == 55.0) and np.all(sqc[8 + rows:] == 55.0)
    return (ysc[1:1 + rows, t], lpc[8:8 + rows], sqc[8:8 + rows], en.cpu().numpy().astype(bool), int(cnt[0]), int(at[0]), seq0)


GRID = [  # V, rows, top_k, top_p, temperature: every value of the issue's table, every pairing that shares a code path
    (1, 1, 0, 1.0, 1.0), (1, 3, 5, 0.9, 2.0),
    (5, 3, 0, 1.0, 0.5), (5, 130, 64, 0.9, 1.0), (5, 3, 2, 0.3, 2.0), (5, 1, 5, 1.0, 1.0),
    (257, 130, 0, 1.0, 2.0), (257, 3, 1, 1.0, 0.5), (257, 130, 5, 0.9, 1.0), (257, 1, 64, 0.3, 0.5), (257, 3, 2, 1.0, 1.0),
    (30522, 130, 0, 1.0, 1.0), (30522, 3, 0, 1.0, 0.5), (30522, 1, 0, 1.0, 2.0), (30522, 130, 5, 0.9, 2.0), (30522, 3, 64, 0.3, 1.0),
    (30522, 1, 1, 1.0, 2.0), (30522, 130, 64, 1.0, 0.5), (30522, 3, 2, 0.9, 1.0), (30522, 130, 64, 0.9, 1.0)]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("V,rows,top_k,top_p,temperature", GRID)
def test_sample_select_matches_the_restatement(V, rows, top_k, top_p, temperature, dtype):
    x, ended, seed, end, (rt, rlp, rended, margin, cut) = _case(V, rows, top_k, top_p, temperature)
    assert (margin <= DELTA).mean() <= 0.01 and np.all(cut > DELTA)
    ctl = _ctl(seed, top_k, temperature, top_p)
    for ldx in ((V + 31) // 32 * 32 + 32, V + 3):        # 16-byte rows (vector loads) and odd rows (element loads), both > V
        tok, lp, sq, en, cnt, at, seq0 = _run_select(x, ended, dtype, ldx, ctl, end)
        again = _run_select(x, ended, dtype, ldx, ctl, end)
        assert np.array_equal(tok, again[0]) and np.array_equal(lp.view(np.int32), again[1].view(np.int32))
        assert np.array_equal(sq.view(np.int32), again[2].view(np.int32))            # a second call: bit-identical
        # ended rows: pad, 0, seq_logp untouched; bookkeeping exact
        assert np.all(tok[ended] == PAD) and np.all(lp[ended] == 0.0) and np.array_equal(sq[ended], seq0[ended])
        want_en = ended | (tok == end)
        assert np.array_equal(en, want_en) and cnt == int(want_en.sum()) and at == (5 if want_en.all() else 8)
        live = ~ended
        assert np.array_equal(sq[live], (seq0[live] + lp[live]).astype(np.float32))
        assert np.all((tok >= 0) & (tok < V))
        # tokens: the restatement's wherever the draw is decided, else its token or the neighbour in candidate order
        same = tok == rt
        bad = [r for r in np.flatnonzero(~same) if margin[r] > DELTA or int(tok[r]) not in S.neighbours(x[r], top_k, int(rt[r]))]
        print(f"V={V} rows={rows} k={top_k} p={top_p} T={temperature} {dtype} ldx={ldx}: {int((~same).sum())} rows differ, "
              f"{int((margin <= DELTA).sum())} undecided, max |dlogp| {np.abs(lp[same] - rlp[same]).max():.3g}")
        assert not bad, (ldx, bad, tok[bad], rt[bad], margin[bad])
        np.testing.assert_allclose(lp[same], rlp[same], rtol=1e-5, atol=1e-6)


def test_out_of_range_settings_are_clamped_on_the_device():
    """top_k beyond 64 acts as 64, a negative one as 0 (the range checks users see are in Python)."""
    x, ended, seed, end, _ = _case(257, 3, 2, 1.0, 1.0)
    for k_dev, k_eq in ((1000, 64), (-4, 0)):
        a = _run_select(x, ended, torch.float32, 260, _ctl(seed, k_dev, 1.0, 1.0), end)
        b = _run_select(x, ended, torch.float32, 260, _ctl(seed, k_eq, 1.0, 1.0), end)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32))


@pytest.mark.parametrize("seed,t", [(0, 1), (0, 29), (12345, 1), (12345, 29)])
def test_distribution(seed, t):
    """65536 identical rows: every empirical frequency within 5 sigma of its probability (independent of the restatement's draw)."""
    from vct_amd import ops
    p = np.array([.5, .25, .125, .0625, .0625])
    n = 65536
    x = torch.from_numpy(np.log(p).astype(np.float32)).to(DEV).repeat(n, 1).contiguous()
    out = torch.full((n,), -1, dtype=torch.long, device=DEV)
    lp, sq = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    en = torch.zeros(n, dtype=torch.uint8, device=DEV)
    cnt, at = torch.zeros(1, dtype=torch.int32, device=DEV), torch.full((1,), 99, dtype=torch.long, device=DEV)
    ws = torch.empty(ops.sample_select_workspace_bytes(torch.float32, n, 5) // 4, dtype=torch.float32, device=DEV)
    ops.sample_select(x, out, -1, PAD, en, cnt, at, t, lp, sq, _ctl(seed, 0, 1.0, 1.0), ws)
    torch.cuda.synchronize()
    tok = out.cpu().numpy()
    freq = np.bincount(tok, minlength=5) / n
    sigma = np.sqrt(p * (1 - p) / n)
    z = (freq - p) / sigma
    print(f"seed {seed} t {t}: z = {np.round(z, 2)}")
    assert freq.size == 5 and np.all(np.abs(z) <= 5.0), z
    np.testing.assert_allclose(lp.cpu().numpy(), np.log(p)[tok], rtol=1e-5, atol=1e-6)
    assert int(cnt[0]) == 0 and int(at[0]) == 99 and not en.any()


def test_sticky_state_over_launches():
    """32 launches on one state and one workspace (never re-initialised, settings alternating between the whole vocabulary and
    top-5): seq_logp is the sum of the step_logp rows, ended rows stay ended, all_ended_at is the first step at which every row
    had ended."""
    from vct_amd import ops
    rows, V, Lmax, end, seed = 7, 257, 40, 9, 4242
    rng = np.random.default_rng(8)
    xs = (rng.integers(-40, 40, (33, rows, V)) / 8.0).astype(np.float32)
    xs[:, :, end] = 3.0                                   # the end token: likely enough that rows end one by one ...
    xs[20:, :, end] = 40.0                                # ... and certain from step 20 on
    ys = torch.full((rows, Lmax), -5, dtype=torch.long, device=DEV)
    lp = torch.full((Lmax, rows), 7.0, dtype=torch.float32, device=DEV)
    sq = torch.zeros(rows, dtype=torch.float32, device=DEV)
    en = torch.zeros(rows, dtype=torch.uint8, device=DEV)
    cnt, at = torch.zeros(1, dtype=torch.int32, device=DEV), torch.full((1,), Lmax, dtype=torch.long, device=DEV)
    ws = torch.full((ops.sample_select_workspace_bytes(torch.float32, rows, V) // 4,), float("nan"), dtype=torch.float32, device=DEV)
    ctls = [_ctl(seed, 0, 1.0, 1.0), _ctl(seed, 5, 1.0, 0.9)]
    xd = torch.from_numpy(xs).to(DEV)
    for t in range(1, 33):
        ops.sample_select(xd[t], ys[:, t], end, PAD, en, cnt, at, t, lp[t], sq, ctls[t % 2], ws)
    torch.cuda.synchronize()
    tok, lpc = ys.cpu().numpy(), lp.cpu().numpy()
    ended = np.zeros(rows, bool)
    acc = np.zeros(rows, np.float32)
    first_all = Lmax
    for t in range(1, 33):
        k, p = ((0, 1.0), (5, 0.9))[t % 2]
        rt, rlp, _, margin, cut = S.select_step(xs[t], ended, seed, t, np.float32(1.0), k, p, PAD, end)
        assert np.all(tok[ended, t] == PAD) and np.all(lpc[t, ended] == 0.0)
        decided = (~ended) & (margin > DELTA) & (cut > DELTA)
        assert np.array_equal(tok[decided, t], rt[decided]), t
        np.testing.assert_allclose(lpc[t, decided], rlp[decided], rtol=1e-5, atol=1e-6)
        acc[~ended] = (acc[~ended] + lpc[t, ~ended]).astype(np.float32)
        ended = ended | (tok[:, t] == end)
        if ended.all() and first_all == Lmax:
            first_all = t
    assert first_all <= 20 and int(at[0]) == first_all and int(cnt[0]) == rows and en.cpu().numpy().all()
    assert np.array_equal(sq.cpu().numpy().view(np.int32), acc.view(np.int32))
    assert np.all(tok[:, 0] == -5) and np.all(tok[:, 33:] == -5) and np.all(lpc[0] == 7.0) and np.all(lpc[33:] == 7.0)


# ---- end to end -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    z = load_golden("tiny_decode.npz")
    mc, V = model_config_of(z), int(z["vocab"])
    cfg = O.cfg_from_model_config(mc, V)
    p = O.init_params(cfg, seed=int(z["param_seed"]))
    return z, build_model(mc, V, DEV, torch.float32, p)


@pytest.fixture(scope="module")
def cfgB():
    """The cfg-B decode fixture (d = 512, V = 30522) in bf16."""
    z = load_golden("cfgB_decode.npz")
    mc, V = model_config_of(z), int(z["vocab"])
    cfg = O.cfg_from_model_config(mc, V)
    p = O.init_params(cfg, seed=int(z["param_seed"]))
    return build_model(mc, V, DEV, torch.bfloat16, p)


def _cfgB_feats(B, seed=5):
    return torch.from_numpy(O.synthetic_batch(B, 12, 512, 20, 30522, seed=seed)[0]).to(DEV)


def _assert_is_greedy(ids, g, N):
    """ids [B, N, L'] against greedy rows g [B*N, L] (the same videos, replicated): equal up to and including each row's first
    end token, pad behind it."""
    ids, g = ids.cpu().numpy(), g.cpu().numpy()
    for r in range(g.shape[0]):
        row = ids[r // N, r % N]
        hits = np.flatnonzero(g[r] == END)
        n = min(hits[0] + 1 if hits.size else g.shape[1], row.size)
        assert np.array_equal(row[:n], g[r, :n]), r
        if hits.size:
            assert np.all(row[n:] == PAD)


@pytest.mark.parametrize("which", ["tiny_fp32", "cfgB_bf16"])
def test_top_k_1_is_greedy(which, tiny, cfgB):
    """top_k = 1, any seed and temperature, N = 2: both samples are the greedy caption.  Greedy runs on the replicated videos, so
    both decodes take the same step variant at the same row count (decode_step_variant)."""
    if which == "tiny_fp32":
        m, feats, max_len = tiny[1], torch.from_numpy(tiny[0]["b3/feats"]).to(DEV), 12
    else:
        m, feats, max_len = cfgB, _cfgB_feats(3, seed=43), 30
    g = m.greedy_decode_ids([feats.repeat_interleave(2, 0)], None, max_len=max_len)
    for seed, temp in ((0, 1.0), (77, 2.0), (5, 0.5)):
        ids, logp = m.sample_decode_ids([feats], None, num_samples=2, max_len=max_len, temperature=temp, top_k=1, seed=seed,
                                        return_logp=True)
        assert ids.dim() == 3 and ids.shape[:2] == (feats.shape[0], 2) and ids.dtype == torch.long
        _assert_is_greedy(ids, g, 2)
        assert torch.all(logp == 0.0) and logp.shape == (feats.shape[0], 2) and logp.dtype == torch.float32


def test_reproducible_and_execution_modes_agree(cfgB):
    from vct_amd import decode, engine
    m = cfgB
    feats = _cfgB_feats(4)
    st = engine.SampleDecodeState(m.cap_decoder._engine(), 4, 3, 13, 30)
    assert engine.decode_step_variant(m.cap_decoder._engine(), st) == "fused"
    run = lambda **kw: decode.sample_decode_ids(m, feats, None, num_samples=3, temperature=1.0, top_k=20, top_p=0.95,
                                                return_logp=True, **kw)
    ids, lp = run(seed=11)
    for other in (run(seed=11), run(seed=11, use_graphs=False)):
        assert torch.equal(ids, other[0]) and torch.equal(lp, other[1])
    # seed=None: torch's default generator decides
    torch.manual_seed(3)
    a = run()
    torch.manual_seed(3)
    b = run()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # rows after their end token hold pad; seq_logp is negative where something was drawn
    idn = ids.cpu().numpy().reshape(12, -1)
    for row in idn:
        hits = np.flatnonzero(row == END)
        if hits.size:
            assert np.all(row[hits[0] + 1:] == PAD)
    assert torch.all(lp < 0)


def test_one_session_serves_every_setting(cfgB):
    """Seed, temperature and top_k are read from the device control block: the captured graphs are reused and each takes effect."""
    from vct_amd import decode
    m = cfgB
    feats = _cfgB_feats(2, seed=8)
    run = lambda seed, temp, k: decode.sample_decode_ids(m, feats, None, num_samples=4, temperature=temp, top_k=k, seed=seed,
                                                         return_logp=True)
    run(1, 2.0, 0)                                       # the first run allocates the steps' buffers, so the next one captures the
    base = run(1, 2.0, 0)                                # begin graph again, as a greedy session's second run does: steady from here
    st = m._decode_sessions[("sample", 2, 4, 13, 30, torch.bfloat16)]
    graphs, begin = dict(st.graphs), st.begin["g"]
    assert len(graphs) >= 1
    others = [run(2, 2.0, 0), run(1, 1.0, 0), run(1, 2.0, 2)]
    for o in others:
        n = min(o[0].shape[2], base[0].shape[2])
        assert not torch.equal(o[0][:, :, :n], base[0][:, :, :n]) or o[0].shape != base[0].shape
        assert not torch.equal(o[1], base[1])
    again = run(1, 2.0, 0)
    assert torch.equal(again[0], base[0]) and torch.equal(again[1], base[1])
    assert m._decode_sessions[("sample", 2, 4, 13, 30, torch.bfloat16)] is st
    assert st.begin["g"] is begin or len(st.graphs) > len(graphs)     # (a position never reached before allocates: begin is re-captured)
    assert all(st.graphs[t] is g for t, g in graphs.items())         # nothing was captured again


@pytest.mark.parametrize("top_k,top_p,temperature", [(0, 1.0, 1.0), (5, 0.9, 2.0)])
def test_fp32_matches_the_reference_algorithm(tiny, top_k, top_p, temperature):
    """KV-cached sampling against the full-decoder re-run with host-side float64 selection, row by row up to each row's first
    undecided step (a cap: at most 10 % of the rows may have one; the seed is chosen so that the reference alone stays within it)."""
    from vct_amd import decode
    z, m = tiny
    feats = torch.from_numpy(z["b3/feats"]).to(DEV)
    kw = dict(max_len=12, num_samples=4, temperature=temperature, top_k=top_k, top_p=top_p, return_logp=True)
    for seed in range(100, 120):
        (rids, rlp), und = decode.sample_decode_ids_reference_algorithm(m, feats, None, seed=seed, **kw)
        if float((und < 12).float().mean()) <= 0.10:
            break
    else:
        raise AssertionError("no seed within the cap found")
    ids, lp = decode.sample_decode_ids(m, feats, None, seed=seed, **kw)
    ids, rids, und = ids.cpu().numpy(), rids.cpu().numpy(), und.cpu().numpy()
    whole = 0
    for b in range(3):
        for n in range(4):
            upto = min(int(und[b, n]), ids.shape[2], rids.shape[2])
            assert np.array_equal(ids[b, n, :upto], rids[b, n, :upto]), (b, n)
            if und[b, n] == 12:
                whole += 1
                assert abs(float(lp[b, n]) - float(rlp[b, n])) <= 1e-4 * max(1.0, abs(float(rlp[b, n])))
    assert whole >= 11                                    # at most 10 % of 12 rows undecided
    assert ids.shape[2] == rids.shape[2] or (und < 12).any()
    # the module API's kv_cache switch reaches the same two functions
    a = m.sample_decode_ids([feats], None, seed=seed, kv_cache=False, **kw)
    assert np.array_equal(a[0].cpu().numpy(), rids)


def test_bf16_follows_the_teacher_forced_logits(cfgB):
    """The sampled ids of a 6-row session, re-derived from the teacher-forced logits of the same KV-cache step at the same row
    count (decode_step_variant) with the restatement and the same uniforms: every token whose margin exceeds DELTA, and seq_logp
    within 1e-4."""
    from vct_amd import decode
    m = cfgB
    B, N, seed = 2, 3, 2024
    feats = _cfgB_feats(B, seed=12)
    for top_k in (0, 5):
        ids, lp = decode.sample_decode_ids(m, feats, None, num_samples=N, temperature=1.0, top_k=top_k, seed=seed, return_logp=True)
        M, Lp = B * N, ids.shape[2]
        flat = ids.reshape(M, Lp)
        _, lg = decode.teacher_forced_next_ids(m, feats.repeat_interleave(N, 0), None, flat, Lp - 1, return_logits=True)
        lg, tok = lg.cpu().numpy(), flat.cpu().numpy()
        ended = np.zeros(M, bool)
        acc = np.zeros(M)
        agree = np.ones(M, bool)
        n_decided = 0
        for t in range(1, Lp):
            rt, rlp, _, margin, _ = S.select_step(lg[:, t - 1], ended, seed, t, np.float32(1.0), top_k, 1.0, PAD, END)
            decided = ended | (margin > DELTA)
            n_decided += int((decided & ~ended).sum())
            assert np.array_equal(tok[decided, t], rt[decided]), (t, tok[:, t], rt, margin)
            agree &= tok[:, t] == rt
            if top_k == 0:
                # the log-probability of the SAMPLED token over the whole vocabulary (whichever side of a boundary the draw fell)
                z = lg[:, t - 1].astype(np.float64)
                zm = z.max(1)
                own = z[np.arange(M), tok[:, t]] - zm - np.log(np.exp(z - zm[:, None]).sum(1))
                acc += np.where(ended, 0.0, own)
            else:
                acc += rlp
            ended = ended | (tok[:, t] == END)
        got = lp.reshape(M).cpu().numpy().astype(np.float64)
        rows_ok = np.ones(M, bool) if top_k == 0 else agree
        print(f"bf16 teacher forced, top_k {top_k}: {n_decided} decided draws, {int(agree.sum())} of {M} rows agree throughout, "
              f"max |seq_logp diff| {np.abs(got - acc)[rows_ok].max():.3g}")
        assert n_decided > 0 and rows_ok.sum() >= M - 1
        assert np.all(np.abs(got - acc)[rows_ok] <= 1e-4)


def test_evaluate_and_module_api(tiny):
    from vct_amd import evaluate
    z, m = tiny
    feats = torch.from_numpy(z["b3/feats"]).to(DEV)
    caps = evaluate.v2t_batch(m, [feats], None, max_len=12, sample=dict(num_samples=2, temperature=2.0, top_k=1, seed=9))
    assert isinstance(caps, list) and len(caps) == 3 and all(isinstance(c, list) and len(c) == 2 for c in caps)
    assert all(isinstance(s, str) for c in caps for s in c)
    greedy = evaluate.v2t_batch(m, [feats.repeat_interleave(2, 0)], None, max_len=12)
    assert [s for c in caps for s in c] == greedy
    one = evaluate.v2t_single(m, [feats[0]], max_len=12, sample=dict(num_samples=3, top_k=8, top_p=0.9, seed=1))
    assert isinstance(one, list) and len(one) == 3 and all(isinstance(s, str) for s in one)
    strs = m.sample_decode([feats], None, num_samples=2, max_len=12, top_k=4, seed=3)
    assert len(strs) == 3 and all(len(c) == 2 for c in strs)
    ids = m.sample_decode_ids([feats], None, num_samples=1, max_len=12, seed=3)
    assert ids.dim() == 3 and ids.shape[:2] == (3, 1) and ids.shape[2] <= 12 and torch.all(ids[:, :, 0] == 101)


def test_greedy_and_beam_never_reach_the_new_wrapper(tiny, monkeypatch):
    from vct_amd import ops
    z, m = tiny
    feats = torch.from_numpy(z["b3/feats"]).to(DEV)
    calls = []
    orig = ops.sample_select
    monkeypatch.setattr(ops, "sample_select", lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
    m.__dict__.pop("_decode_sessions", None)             # fresh sessions: every step is issued (and captured) under the spy
    m.greedy_decode_ids([feats], None, max_len=12)
    m.greedy_decode_ids([feats[:1]], None, max_len=12)
    m.beam_decode_ids([feats], None, beam_size=3, max_len=12)
    assert calls == []
    m.sample_decode_ids([feats], None, num_samples=2, max_len=12, seed=1)
    assert calls                                          # (the spy works)
