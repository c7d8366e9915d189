"""Generation controls on the device (csrc/vct_logit_controls.hip, DecodeState.apply_controls, decode.GenerationControls): the kernel
through ops.logit_controls bit for bit against the numpy restatement (tests/gen_controls_ref.py) over the whole logits matrix, in
row and beam form; decoding end to end on a model whose logits are planted (ids predicted by a host simulation); and a real
model, every step's processed logits against decode.apply_controls_host."""
import functools

import numpy as np
import pytest
import torch

import gen_controls_ref as R
import vct_oracle as O
from helpers import build_model, load_golden, model_config_of

pytestmark = pytest.mark.gpu
DEV = "cuda"
START, END, PAD = 101, 102, 0
LMAX = 65


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _ctl(min_length=0, n=0, theta=1.0, banned_ids=()):
    return torch.frombuffer(bytearray(R.pack(min_length, n, theta, tuple(banned_ids))), dtype=torch.int32).to(DEV)


def _same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    it = torch.int16 if a.dtype == torch.bfloat16 else torch.int32
    return a.dtype == b.dtype and torch.equal(a.contiguous().view(it), b.contiguous().view(it))


def _combos(rows):
    """(t, n, theta, min_length, banned): t in {1, 2, n-1, n, 63, 64} for every n in {0, 1, 2, 3, 8}, theta in {1, 1.5, 2};
    min_length and the banned list (duplicates, the end token among them) alternate over the combinations."""
    out, i = [], 0
    for n in (0, 1, 2, 3, 8):
        for t in sorted({1, 2, n - 1, n, 63, 64} & set(range(1, 65))):
            for theta in (1.0, 1.5, 2.0):
                m = (0, t, t - 1)[i % 3]
                out.append((t, n, theta, m, i % 2 == 1))
                i += 1
    return out


@functools.lru_cache(maxsize=None)
def _matrix(rows, V, seed):
    """Logits on a 1/8 grid (exact in bf16) with pad columns poisoned, an alphabet of 4 tokens (the end token among them) whose
    logits are positive, negative and zero over the rows, ids over the first 3 to 4 of them, every third row ended."""
    rng = np.random.default_rng(seed)
    ld = V + 10
    x = (rng.integers(-80, 80, (rows, ld)) / 8.0).astype(np.float32)
    x[:, V:] = 1e4
    alpha = np.array([END % V if V > END else 5, 7, V - 1, 33], np.int64)
    for r in range(rows):
        for k, v in enumerate(alpha):
            x[r, v] = (2.625, -1.875, 0.0, -0.0, 7.5)[(r + k) % 5]
    width = 3 + (np.arange(rows) % 2)                                   # 3- and 4-token alphabets
    ids = alpha[rng.integers(0, 1 << 30, (rows, LMAX)) % width[:, None]]
    ended = np.arange(rows) % 3 == 2
    banned = (int(alpha[1]), int(alpha[1]), int(alpha[0]), int(rng.integers(0, V)))
    return x, ids, ended, int(alpha[0]), banned


@pytest.mark.parametrize("rows", [1, 3, 130])
@pytest.mark.parametrize("V", [70, 1000, 30522])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_kernel_equals_the_restatement(dtype, V, rows):
    from vct_amd import ops
    x, ids, ended, end, banned_all = _matrix(rows, V, 7 * V + rows)
    bf = dtype == torch.bfloat16
    xd = torch.from_numpy(x).to(DEV, dtype)
    xin = xd.float().cpu().numpy()                                      # what the kernel sees (the poison rounded to the dtype)
    idd, end_d = torch.from_numpy(ids).to(DEV), torch.from_numpy(ended).to(DEV)
    for i, (t, n, theta, m, with_banned) in enumerate(_combos(rows)):
        banned = banned_all if with_banned else ()
        want = R.apply(xin, ids[:, :t].tolist(), end, ended, bf, min_length=m, n=n, theta=theta, banned_ids=banned)
        got = xd.clone()
        ops.logit_controls(got[:, :V], idd, end_d, _ctl(m, n, theta, banned), t, end, cols=V)
        assert _same_bits(got, torch.from_numpy(want).to(DEV, dtype)), (t, n, theta, m, banned)
        assert _same_bits(got[ended], xd[ended]) and _same_bits(got[:, V:], xd[:, V:])
        if i % 7 == 0:                                                  # a second run on the same input: the same bits
            again = xd.clone()
            ops.logit_controls(again[:, :V], idd, end_d, _ctl(m, n, theta, banned), t, end, cols=V)
            assert _same_bits(again, got)


@pytest.mark.parametrize("K", [1, 3, 16])
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("V", [70, 30522])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_beam_kernel_equals_the_back_tracked_restatement(dtype, V, B, K):
    from vct_amd import ops
    M = B * K
    x, tokens, finished, end, banned_all = _matrix(M, V, 11 * V + 100 * B + K)
    rng = np.random.default_rng(K + 17 * B)
    parents = np.zeros((LMAX, M), np.int32)
    for s in range(LMAX):
        for b in range(B):
            parents[s, b * K:(b + 1) * K] = b * K + rng.permutation(K)
    bf = dtype == torch.bfloat16
    xd = torch.from_numpy(x).to(DEV, dtype)
    xin = xd.float().cpu().numpy()
    tok_d, fin_d, par_d = torch.from_numpy(tokens).to(DEV), torch.from_numpy(finished).to(DEV).to(torch.uint8), torch.from_numpy(parents).to(DEV)
    for i, (t, n, theta, m, with_banned) in enumerate(_combos(M)):
        banned = banned_all if with_banned else ()
        want = R.apply_beam(xin, tokens, parents, t, end, finished, bf, min_length=m, n=n, theta=theta, banned_ids=banned)
        got = xd.clone()
        ops.logit_controls(got[:, :V], tok_d, fin_d, _ctl(m, n, theta, banned), t, end, cols=V, parents=par_d, K=K)
        assert _same_bits(got, torch.from_numpy(want).to(DEV, dtype)), (t, n, theta, m, banned)
        if i % 7 == 0:
            again = xd.clone()
            ops.logit_controls(again[:, :V], tok_d, fin_d, _ctl(m, n, theta, banned), t, end, cols=V, parents=par_d, K=K)
            assert _same_bits(again, got)
    if K > 1:       # the histories do follow the parents: the rows of the token table give another answer
        assert not np.array_equal(R.apply(xin, tokens[:, :40].tolist(), end, finished, bf, n=2, theta=2.0),
                                  R.apply_beam(xin, tokens, parents, 40, end, finished, bf, n=2, theta=2.0))


def test_kernel_refusals_raise():
    from vct_amd import ops
    x = torch.zeros(6, 80, device=DEV)
    ids = torch.zeros(6, LMAX, dtype=torch.long, device=DEV)
    ended = torch.zeros(6, dtype=torch.bool, device=DEV)
    par = torch.zeros(LMAX, 6, dtype=torch.int32, device=DEV)
    ctl = _ctl()
    for kw in (dict(t=0), dict(t=65), dict(t=3, parents=par, K=17), dict(t=3, parents=par, K=0), dict(t=3, parents=par, K=4)):
        with pytest.raises(ValueError, match="VCT_E_SHAPE"):
            ops.logit_controls(x[:, :70], ids, ended, ctl, kw.pop("t"), END, cols=70, **kw)
    with pytest.raises(ValueError, match="VCT_E_SHAPE"):
        ops.logit_controls(x[:, :70], ids, ended, ctl, 3, END, cols=90)       # ldx < V
    with pytest.raises(TypeError):
        ops.logit_controls(x.half()[:, :70], ids, ended, ctl, 3, END, cols=70)
    torch.cuda.synchronize()
    assert float(x.abs().sum()) == 0.0


# ---- end to end, exact by construction: generator.weight = 0, the logits ARE the planted bias -------------------------------------
A, Bt, C = 10, 20, 30
PLANTS = {"end_high": {A: 4.0, Bt: 3.5, C: 3.25, END: 5.0}, "end_low": {A: 4.0, Bt: 3.5, C: 3.25, END: 3.0}}
REST = -1.0


def _planted(name, dtype):
    z = load_golden(name)
    mc, V = model_config_of(z), int(z["vocab"])
    p = O.init_params(O.cfg_from_model_config(mc, V), seed=int(z["param_seed"]))
    p["cap_decoder.generator.weight"] = np.zeros_like(p["cap_decoder.generator.weight"])
    return build_model(mc, V, DEV, dtype, p), V


def _plant(m, plant):
    bias = np.full(m.cap_decoder._engine().V, REST, np.float32)
    for k, v in PLANTS[plant].items():
        bias[k] = v
    with torch.no_grad():
        m.load_state_dict({"cap_decoder.generator.bias": torch.from_numpy(bias)}, strict=False)
    return bias


@pytest.fixture(scope="module")
def tiny_planted():
    return _planted("tiny_decode.npz", torch.float32)


@pytest.fixture(scope="module")
def cfgB_planted():
    return _planted("cfgB_decode.npz", torch.bfloat16)


def _simulate(bias, max_len, bf16=False, **ctl):
    """Greedy decoding of one row whose logits are `bias` at every step: the ids up to the stop, then the row's end step."""
    h, ended = [START], False
    for t in range(1, max_len):
        x = bias.copy()
        if not ended:
            R.apply_row(x, h, END, bf16=bf16, **ctl)
        h.append(int(np.argmax(x)))
        ended = ended or h[-1] == END
        if ended:
            break
    return h


CASES = [("end_high", dict(min_length=4)), ("end_high", dict(min_length=7, n=2)), ("end_low", dict(theta=2.0)),
         ("end_low", dict(n=1, min_length=5)), ("end_low", dict(banned_ids=(A, C, A))), ("end_high", dict(banned_ids=(END, Bt), min_length=0)),
         ("end_high", dict(min_length=9, n=3, theta=1.5, banned_ids=(Bt,))), ("end_low", dict(min_length=6, n=2, theta=2.0, banned_ids=(C,)))]


def _controls(kw):
    from vct_amd.decode import GenerationControls
    return GenerationControls(kw.get("min_length", 0), kw.get("n", 0), kw.get("theta", 1.0), kw.get("banned_ids", ()))


def _feats(m, B, seed=0):
    T, E = 5, m.model_config["modal_shape"][0]
    return torch.from_numpy(np.random.default_rng(seed).standard_normal((B, T, E)).astype(np.float32)).to(DEV)


def test_planted_cases_exercise_every_rule():
    bias = np.full(131, REST, np.float32)
    seen = set()
    for plant, kw in CASES:
        b = bias.copy()
        for k, v in PLANTS[plant].items():
            b[k] = v
        seen.add(tuple(_simulate(b, 14, **kw)))
        assert _simulate(b, 14, **kw) != _simulate(b, 14)
    assert len(seen) == len(CASES)


@pytest.mark.parametrize("B", [1, 3])
def test_planted_greedy_and_top1_sampling(tiny_planted, B):
    from vct_amd import decode
    m, V = tiny_planted
    feats, max_len = _feats(m, B), 14
    for plant, kw in CASES:
        bias = _plant(m, plant)
        want = _simulate(bias, max_len, **kw)
        c = _controls(kw)
        ys = decode.greedy_decode_ids(m, feats, None, max_len, controls=c)
        assert ys.cpu().tolist() == [want] * B, (plant, kw)
        assert torch.equal(ys, decode.greedy_decode_ids(m, feats, None, max_len, controls=c, use_graphs=False))
        assert torch.equal(ys, decode.greedy_decode_ids_reference_algorithm(m, feats, None, max_len, controls=c))
        ids, lp = decode.sample_decode_ids(m, feats, None, max_len, num_samples=2, top_k=1, seed=3, controls=c, return_logp=True)
        assert ids.cpu().tolist() == [[want] * 2] * B and torch.all(lp == 0.0)
        assert torch.equal(ids, decode.sample_decode_ids(m, feats, None, max_len, num_samples=2, top_k=1, seed=3, controls=c, use_graphs=False))
        ref = decode.sample_decode_ids_reference_algorithm(m, feats, None, max_len, num_samples=2, top_k=1, seed=3, controls=c)[0]
        assert torch.equal(ids, ref)


def test_planted_greedy_batch_1_takes_the_gemv_step(cfgB_planted):
    from vct_amd import decode, engine
    m, V = cfgB_planted
    eng = m.cap_decoder._engine()
    feats, max_len = _feats(m, 1), 14
    for plant, kw in CASES[1:3] + CASES[6:]:
        bias = _plant(m, plant)
        c = _controls(kw)
        ys = decode.greedy_decode_ids(m, feats, None, max_len, controls=c)
        assert ys.cpu().tolist() == [_simulate(bias, max_len, **kw)], (plant, kw)
        assert torch.equal(ys, decode.greedy_decode_ids(m, feats, None, max_len, controls=c, use_graphs=False))
        plain = decode.greedy_decode_ids(m, feats, None, max_len)
        assert plain.cpu().tolist() == [_simulate(bias, max_len)]
    sessions = m.__dict__["_decode_sessions"]
    with_ctl = [st for k, st in sessions.items() if "ctl" in k]
    without = [st for k, st in sessions.items() if "ctl" not in k]
    assert len(with_ctl) == 1 and len(without) == 1
    assert engine.decode_step_variant(eng, with_ctl[0]) == "gemv" and engine.decode_step_variant(eng, without[0]) == "block"
    # batch 3 in bf16: the fused step, logits in bf16
    feats3 = _feats(m, 3)
    plant, kw = CASES[7]
    bias = _plant(m, plant)
    ys = decode.greedy_decode_ids(m, feats3, None, max_len, controls=_controls(kw))
    assert ys.cpu().tolist() == [_simulate(bias, max_len, bf16=True, **kw)] * 3
    st3 = [st for k, st in sessions.items() if "ctl" in k and st.B == 3]
    assert len(st3) == 1 and engine.decode_step_variant(eng, st3[0]) == "fused" and st3[0].last_logits.dtype == torch.bfloat16


def test_planted_beams_equal_the_reference_algorithm(tiny_planted):
    from vct_amd import decode
    m, V = tiny_planted
    feats, max_len, K = _feats(m, 2), 12, 3
    for plant, kw in CASES:
        _plant(m, plant)
        c = _controls(kw)
        (ids_ref, fin_ref), margin = decode.beam_decode_ids_reference_algorithm(m, feats, None, K, max_len, return_all=True, controls=c)
        print("beam margin", plant, kw, margin)
        assert margin == 0.0 or margin > 1e-3, margin          # exact ties (to the smaller flat index) or clear gaps, nothing between
        ids, fin = decode.beam_decode_ids(m, feats, None, K, max_len, return_all=True, controls=c)
        assert torch.equal(ids, ids_ref), (plant, kw)
        torch.testing.assert_close(fin, fin_ref, rtol=1e-5, atol=1e-5)
        ids2, fin2 = decode.beam_decode_ids(m, feats, None, K, max_len, return_all=True, controls=c, use_graphs=False)
        assert torch.equal(ids, ids2) and torch.equal(fin, fin2)
        # the rules hold along every beam
        for row in ids.reshape(-1, ids.shape[-1]).cpu().tolist():
            cut = row[:row.index(END) + 1] if END in row else row
            assert not (set(cut) & set(kw.get("banned_ids", ()))) and (END not in row or row.index(END) > kw.get("min_length", 0))


def test_one_session_serves_every_setting(tiny_planted):
    from vct_amd import decode
    m, V = tiny_planted
    feats, max_len = _feats(m, 3), 14
    bias = _plant(m, "end_low")
    m.__dict__.pop("_decode_sessions", None)
    first = decode.greedy_decode_ids(m, feats, None, max_len, controls=_controls(dict(min_length=max_len - 2, n=2)))
    assert first.cpu().tolist() == [_simulate(bias, max_len, min_length=max_len - 2, n=2)] * 3 and first.shape[1] == max_len
    (key, st), = m.__dict__["_decode_sessions"].items()
    assert "ctl" in key and len(st.graphs) == max_len - 1
    graphs = dict(st.graphs)
    for kw in (dict(theta=2.0), dict(banned_ids=(A, Bt)), dict(min_length=3, n=1, theta=1.5, banned_ids=(C,))):
        ys = decode.greedy_decode_ids(m, feats, None, max_len, controls=_controls(kw))
        assert ys.cpu().tolist() == [_simulate(bias, max_len, **kw)] * 3, kw
        assert m.__dict__["_decode_sessions"][key] is st and st.graphs == graphs and len(st.graphs) == max_len - 1


def test_no_controls_means_no_launch(tiny_planted, monkeypatch):
    from vct_amd import decode, ops
    m, V = tiny_planted
    _plant(m, "end_low")
    feats, max_len = _feats(m, 2), 10
    m.__dict__.pop("_decode_sessions", None)
    runs = {"greedy": lambda **kw: decode.greedy_decode_ids(m, feats, None, max_len, **kw),
            "beam": lambda **kw: decode.beam_decode_ids(m, feats, None, 3, max_len, **kw),
            "sample": lambda **kw: decode.sample_decode_ids(m, feats, None, max_len, num_samples=2, top_k=5, seed=9, **kw)}
    before = {k: f() for k, f in runs.items()}
    sessions = dict(m.__dict__["_decode_sessions"])
    assert len(sessions) == 3

    def boom(*a, **kw):
        raise AssertionError("vct_logit_controls launched without controls")
    monkeypatch.setattr(ops, "logit_controls", boom)
    for kw in (dict(), dict(controls=None), dict(controls=decode.GenerationControls())):
        for k, f in runs.items():
            assert torch.equal(f(**kw), before[k]), (k, kw)
            assert torch.equal(f(use_graphs=False, **kw), before[k]), (k, kw)
    now = m.__dict__["_decode_sessions"]
    assert set(now) == set(sessions) and all(now[k] is sessions[k] for k in sessions)
    assert all(st.gen_ctl is None for st in now.values())
    with pytest.raises(AssertionError, match="without controls"):
        decode.greedy_decode_ids(m, feats, None, max_len, controls=decode.GenerationControls(min_length=2), use_graphs=False)


# ---- a real model -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    z = load_golden("tiny_decode.npz")
    mc, V = model_config_of(z), int(z["vocab"])
    p = O.init_params(O.cfg_from_model_config(mc, V), seed=int(z["param_seed"]))
    return z, build_model(mc, V, DEV, torch.float32, p), V


def _record(monkeypatch, V, controls):
    """Wrap ops.logit_controls: every call's raw logits go through decode.apply_controls_host with the history the call itself
    names (beams: back-tracked on the host) and must equal what the kernel left, bit for bit.  Returns the per-step records."""
    from vct_amd import decode, ops
    real, steps = ops.logit_controls, []

    def wrapped(x, ids, ended, ctl, t, end_id, cols=None, parents=None, K=0):
        raw = x.clone()
        real(x, ids, ended, ctl, t, end_id, cols=cols, parents=parents, K=K)
        if parents is None:
            hist = ids[:, :t].clone()
        else:
            tk, pr = ids.cpu().numpy(), parents.cpu().numpy()
            hist = torch.tensor([R.backtrack(tk, pr, r, t) for r in range(x.shape[0])], dtype=torch.long)
        host = decode.apply_controls_host(raw.clone(), hist, end_id, controls, ended.clone(), V=cols)
        assert cols == V and _same_bits(host, x), t
        steps.append((t, x.float().cpu().numpy(), ended.cpu().numpy().astype(bool)))
    monkeypatch.setattr(ops, "logit_controls", wrapped)
    return steps


def _check_caption(row, banned, min_length):
    cut = row[:row.index(END) + 1] if END in row else row
    grams = list(zip(cut, cut[1:]))
    assert len(grams) == len(set(grams)), cut                      # no bigram twice
    assert END not in row[1:min_length + 1], row                   # no end token before column min_length + 1
    assert banned not in cut, cut
    return cut


def _real_case(tiny):
    from vct_amd import decode
    z, m, V = tiny
    feats, max_len = torch.from_numpy(z["b3/feats"]).to(DEV), 12
    plain = decode.greedy_decode_ids(m, feats, None, max_len).cpu().tolist()
    banned = next(v for v in plain[0][1:] if v not in (START, END, PAD))         # a token the uncontrolled run emits
    assert any(END in row[1:6] for row in plain)                                 # ... and it ends before column 6
    return m, V, feats, max_len, plain, banned, decode.GenerationControls(min_length=5, no_repeat_ngram_size=2, banned_ids=(banned,))


def test_real_model_greedy(tiny, monkeypatch):
    """Every step's token is the first arg-max of the processed logits, which are apply_controls_host of the raw ones."""
    from vct_amd import decode
    m, V, feats, max_len, plain, banned, c = _real_case(tiny)
    want = decode.greedy_decode_ids(m, feats, None, max_len, controls=c)
    assert want.cpu().tolist() != plain
    steps = _record(monkeypatch, V, c)
    ys = decode.greedy_decode_ids(m, feats, None, max_len, controls=c, use_graphs=False)
    assert torch.equal(ys, want)
    ysn = ys.cpu().numpy()
    assert len(steps) >= ysn.shape[1] - 1 and [s[0] for s in steps] == list(range(1, len(steps) + 1))
    for t, x, ended in steps[:ysn.shape[1] - 1]:
        assert np.array_equal(ysn[:, t], np.argmax(x[:, :V], axis=1)), t
    for row in ysn.tolist():
        _check_caption(row, banned, 5)
    assert m.greedy_decode_ids([feats], None, max_len=max_len, controls=c).cpu().tolist() == ysn.tolist()


def test_real_model_sampled_top_1(tiny, monkeypatch):
    """top_k = 1: the arg-max of the processed logits for every live row, pad behind the end."""
    from vct_amd import decode
    m, V, feats, max_len, plain, banned, c = _real_case(tiny)
    want = decode.sample_decode_ids(m, feats, None, max_len, num_samples=2, top_k=1, seed=1, controls=c)
    steps = _record(monkeypatch, V, c)
    ids = decode.sample_decode_ids(m, feats, None, max_len, num_samples=2, top_k=1, seed=1, controls=c, use_graphs=False)
    assert torch.equal(ids, want)
    flat = ids.reshape(6, -1).cpu().numpy()
    assert len(steps) >= flat.shape[1] - 1
    for t, x, ended in steps[:flat.shape[1] - 1]:
        live = ~ended
        assert np.array_equal(flat[live, t], np.argmax(x[live, :V], axis=1)) and np.all(flat[~live, t] == PAD), t
    for row in flat.tolist():
        _check_caption(row, banned, 5)


def test_real_model_beams(tiny, monkeypatch):
    """The processed logits of every step are the host's for the back-tracked histories (checked inside the wrapper); the rules
    hold along every beam."""
    from vct_amd import decode
    m, V, feats, max_len, plain, banned, c = _real_case(tiny)
    want = decode.beam_decode_ids(m, feats, None, 3, max_len, controls=c, return_all=True)[0]
    steps = _record(monkeypatch, V, c)
    beams = decode.beam_decode_ids(m, feats, None, 3, max_len, controls=c, return_all=True, use_graphs=False)[0]
    assert torch.equal(beams, want) and len(steps) >= beams.shape[-1] - 1
    for row in beams.reshape(9, -1).cpu().tolist():
        _check_caption(row, banned, 5)
    (ref, _), margin = decode.beam_decode_ids_reference_algorithm(m, feats, None, 3, max_len, return_all=True, controls=c)
    if margin > 1e-4:
        assert torch.equal(beams, ref)


class _Loader:
    """A by_video loader of one batch, with its references."""

    class _Dataset:
        video2caption = {"v0": [[START, 5, 6, END]], "v1": [[START, 7, END]], "v2": [[START, 8, 9, 10, END]]}

        def __len__(self):
            return 3

    def __init__(self, feats):
        self.dataset, self.feats = self._Dataset(), feats

    def __iter__(self):
        yield [self.feats], None, None, ["v0", "v1", "v2"]


@pytest.mark.parametrize("beam", [None, 3])
def test_evaluate_passes_controls_on(tiny, beam):
    """v2t_batch, eval_epoch and eval_metrics with controls= give the captions of the direct call's ids."""
    from vct_amd import decode, evaluate
    z, m, V = tiny
    feats, max_len = torch.from_numpy(z["b3/feats"]).to(DEV), 12
    c = decode.GenerationControls(min_length=5, no_repeat_ngram_size=2, repetition_penalty=1.2)
    direct = (lambda **kw: m.greedy_decode_ids([feats], None, max_len=max_len, **kw)) if beam is None else \
        (lambda **kw: m.beam_decode_ids([feats], None, beam_size=beam, max_len=max_len, **kw))
    ids = direct(controls=c)
    assert ids.cpu().tolist() != direct().cpu().tolist()
    caps = [evaluate._strip_special(s) for s in m._ids_to_captions(ids)]
    assert evaluate.v2t_batch(m, [feats], None, max_len=max_len, beam_size=beam, controls=c) == caps
    scores, got = evaluate.eval_metrics(m, _Loader(feats), max_len=max_len, beam_size=beam, return_captions=True, controls=c)
    assert list(got.values()) == caps and "CIDEr" in scores
    assert evaluate.eval_epoch(m, _Loader(feats), max_len=max_len, beam_size=beam, controls=c) == got


def test_evaluate_sampled_attention_and_single(tiny):
    from vct_amd import decode, evaluate
    z, m, V = tiny
    feats, max_len = torch.from_numpy(z["b3/feats"]).to(DEV), 12
    c = decode.GenerationControls(min_length=5, no_repeat_ngram_size=2, repetition_penalty=1.2)
    strip = lambda caps: [evaluate._strip_special(s) for s in caps]
    smp = dict(num_samples=2, top_k=3, temperature=0.7, seed=4)
    direct = m.sample_decode_ids([feats], None, max_len=max_len, controls=c, **smp)
    sm = evaluate.v2t_batch(m, [feats], None, max_len=max_len, sample=smp, controls=c)
    assert [cap for caps in sm for cap in caps] == strip(m._ids_to_captions(direct.reshape(6, -1)))
    ys = m.greedy_decode_ids([feats], None, max_len=max_len, controls=c)
    caps, maps = evaluate.v2t_batch(m, [feats], None, max_len=max_len, return_attn=True, controls=c)
    assert caps == strip(m._ids_to_captions(ys)) and maps.shape[2] == ys.shape[1] - 1
    assert evaluate.v2t_single(m, [feats[0]], max_len=max_len, controls=c) == \
        strip(m._ids_to_captions(m.greedy_decode_ids([feats[:1]], None, max_len=max_len, controls=c)))[0]
