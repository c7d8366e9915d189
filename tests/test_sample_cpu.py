"""CPU-side checks of sampled decoding: the numpy restatement (tests/sample_ref.py) on hand-worked cases, the uniform stream
against recorded values, every Python refusal (model on "cpu": no device is touched) and the entry point's argument codes."""
import ctypes
import math

import numpy as np
import pytest
import torch

import sample_ref as S
import vct_oracle as O
from helpers import build_model, load_golden, model_config_of

END, PAD = 102, 0


# ---- the uniform stream ------------------------------------------------------------------------------------------------------
def test_uniform_recorded_values():
    """Values generated with the restatement; the package's host copy (plain Python integers) must give the same stream."""
    from vct_amd import decode
    rec = {(0, 3, 1): [0.9286749362945557, 0.8251729607582092, 0.22101902961730957],
           (12345, 2, 29): [0.4126526117324829, 0.4976983070373535],
           (2 ** 31 - 1, 4, 2): [0.5298783779144287, 0.854575514793396, 0.45469212532043457, 0.28482872247695923],
           (1, 1, 0): [0.37505078315734863]}
    for (seed, rows, t), want in rec.items():
        assert S.uniform(seed, rows, t).tolist() == want
        assert decode.sample_uniforms(seed, rows, t) == want
    u = S.uniform(3, 4096, 5)
    assert u.min() >= 0.0 and u.max() < 1.0 and np.all(u * 2 ** 24 == np.round(u * 2 ** 24))


def test_uniform_by_hand():
    """Seed 0, rows 3, t 1, row 2, spelled out: key = (0 * 0x9E3779B1) ^ (997 * 0x85EBCA77 + 0x165667B1) mod 2^32."""
    M = 0xFFFFFFFF

    def h(x):
        x ^= x >> 16
        x = (x * 0x85EBCA6B) & M
        x ^= x >> 13
        x = (x * 0xC2B2AE35) & M
        return x ^ (x >> 16)
    key = 0 ^ ((997 * 0x85EBCA77 + 0x165667B1) & M)
    assert key == (997 * 2246822519 + 374761393) % 2 ** 32
    idx = 1 * 3 + 2
    hv = h((h(key) + idx * 0x9E3779B1) & M)
    assert (hv >> 8) / 2 ** 24 == S.uniform(0, 3, 1)[2] == 0.22101902961730957


def test_engine_names_the_site():
    from vct_amd import engine
    assert engine.SAMPLE_SITE == S.SITE == 997
    assert engine.SAMPLE_SITE not in (engine.ENC_IN_SITE, engine.EMB_SITE) and engine.SAMPLE_SITE < engine.DEC_SITE


# ---- the restatement on hand-worked cases ----------------------------------------------------------------------------------------
def test_single_token_vocabulary():
    x = np.array([[3.5], [-2.0]], np.float32)
    for k in (0, 1, 64):
        tok, lp, ended, margin, _ = S.select_step(x, np.zeros(2, bool), 5, 1, 0.5, k, 1.0, PAD, 0)
        assert tok.tolist() == [0, 0] and lp.tolist() == [0.0, 0.0] and ended.all()


def test_k1_is_first_index_argmax():
    x = np.array([[1.0, 4.0, 4.0, -1.0], [2.0, 2.0, 2.0, 2.0], [0.0, -1.0, 5.0, 5.0]], np.float32)
    for seed in range(5):
        tok, lp, ended, _, _ = S.select_step(x, np.zeros(3, bool), seed, 3, 2.0, 1, 1.0, PAD, 2)
        assert tok.tolist() == [1, 0, 2] and lp.tolist() == [0.0, 0.0, 0.0]
        assert ended.tolist() == [False, False, True]


def test_five_token_row_draw_by_draw():
    p = np.array([.5, .25, .125, .0625, .0625])
    x = np.log(np.tile(p, (8, 1))).astype(np.float32)
    edges = [0.5, 0.75, 0.875, 0.9375, 1.0]
    tok, lp, ended, margin, cut = S.select_step(x, np.zeros(8, bool), 7, 3, 1.0, 0, 1.0, PAD, 4)
    u = S.uniform(7, 8, 3)
    np.testing.assert_allclose(u, [0.43321127, 0.63637114, 0.8875947, 0.63204193, 0.18715703, 0.87499118, 0.58619559, 0.38838053],
                               atol=5e-9)
    assert tok.tolist() == [0, 1, 3, 1, 0, 2, 1, 0]                       # each u against the edges above, by eye
    for r in range(8):
        c = next(i for i, e in enumerate(edges) if u[r] < e)
        assert tok[r] == c
        assert abs(lp[r] - math.log(p[c])) < 1e-6
        lo = 0.0 if c == 0 else edges[c - 1]
        assert abs(margin[r] - min(u[r] - lo, edges[c] - u[r])) < 1e-7
    assert margin[5] < 1e-5 < margin[4]                                    # row 5 sits 8.8e-6 below the 0.875 edge
    assert not ended.any() and np.all(np.isinf(cut))
    # temperature 0.5 squares the weights: p^2 / sum(p^2)
    q = p ** 2 / (p ** 2).sum()
    tok2, lp2, _, _, _ = S.select_step(x, np.zeros(8, bool), 7, 3, 2.0, 0, 1.0, PAD, 4)
    for r in range(8):
        assert tok2[r] == int(np.searchsorted(np.cumsum(q), u[r], side="right"))
        assert abs(lp2[r] - math.log(q[tok2[r]])) < 1e-6
    # an ended row: pad, 0, flags untouched
    e0 = np.array([True] + [False] * 7)
    tok3, lp3, e3, m3, _ = S.select_step(x, e0, 7, 3, 1.0, 0, 1.0, PAD, 4)
    assert tok3[0] == PAD and lp3[0] == 0.0 and e3[0] and np.isinf(m3[0]) and tok3[1:].tolist() == tok[1:].tolist()


def test_top_k_order_nucleus_and_clip():
    # rank order with ties to the smaller index: columns 3, 1, 4 (tie 2.0: 1 before 4), 0, 2
    x = np.array([[1.0, 2.0, -1.0, 3.0, 2.0]], np.float32)
    assert S.candidates(x[0], 3).tolist() == [3, 1, 4] and S.candidates(x[0], 64).tolist() == [3, 1, 4, 0, 2]
    w = np.exp(np.array([3.0, 2.0, 2.0]) - 3.0)
    for seed in range(20):
        u = S.uniform(seed, 1, 2)[0]
        tok, lp, _, _, _ = S.select_step(x, np.zeros(1, bool), seed, 2, 1.0, 3, 1.0, PAD, END)
        c = int(np.searchsorted(np.cumsum(w) / w.sum(), u, side="right"))
        assert tok[0] == [3, 1, 4][c] and abs(lp[0] - math.log(w[c] / w.sum())) < 1e-12
        # a nucleus so small that only the best candidate stays
        tok, lp, _, _, cut = S.select_step(x, np.zeros(1, bool), seed, 2, 1.0, 5, 1e-3, PAD, END)
        assert tok[0] == 3 and lp[0] == 0.0 and np.isfinite(cut[0])
        # top_p = 0.8 of the top 3: shares 0.576, 0.788, 1 -> all three stay; 0.7 -> two stay
        tok, lp, _, _, _ = S.select_step(x, np.zeros(1, bool), seed, 2, 1.0, 3, 0.7, PAD, END)
        c = 0 if u * (w[0] + w[1]) < w[0] else 1
        assert tok[0] == [3, 1][c] and abs(lp[0] - math.log(w[c] / (w[0] + w[1]))) < 1e-12
        # k > V is clipped to V
        a = S.select_step(x, np.zeros(1, bool), seed, 2, 1.0, 64, 0.9, PAD, END)
        b = S.select_step(x, np.zeros(1, bool), seed, 2, 1.0, 5, 0.9, PAD, END)
        assert a[0].tolist() == b[0].tolist() and a[1].tolist() == b[1].tolist()


def test_generator_margin_cap_holds_on_the_restatement():
    """The share of rows within delta = 1e-5 of a boundary is far below the 1 % cap on the GPU tests' kind of input."""
    rng = np.random.default_rng(0)
    x = (rng.integers(-80, 80, (130, 257)) / 8.0).astype(np.float32)
    for k, p in ((0, 1.0), (5, 0.9), (64, 0.3)):
        margin = S.select_step(x, np.zeros(130, bool), 11, 4, 1.0, k, p, PAD, END)[3]
        assert (margin <= 1e-5).mean() <= 0.01


# ---- Python refusals: nothing touches a device -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cpu_model():
    z = load_golden("tiny_decode.npz")
    mc, V = model_config_of(z), int(z["vocab"])
    cfg = O.cfg_from_model_config(mc, V)
    return build_model(mc, V, "cpu", torch.float32, O.init_params(cfg, seed=int(z["param_seed"]))), z


def test_refusals(cpu_model, monkeypatch):
    from vct_amd import decode, evaluate, ops
    m, z = cpu_model
    feats = torch.from_numpy(z["b3/feats"])

    def boom(*a, **k):
        raise AssertionError("device work before the argument checks")
    monkeypatch.setattr(decode.cached, "_run_session", boom)
    monkeypatch.setattr(decode.cached, "_session", boom)
    monkeypatch.setattr(ops, "sample_select", boom)
    bad = [dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float("inf")), dict(temperature=float("nan")),
           dict(top_k=-1), dict(top_k=65), dict(top_k=2.5), dict(top_p=0.0), dict(top_p=1.5), dict(top_p=-0.1, top_k=5),
           dict(top_p=0.9), dict(top_p=0.9, top_k=0), dict(num_samples=0), dict(num_samples=-2)]
    for kw in bad:
        for fn in (lambda **k: decode.sample_decode_ids(m, feats, None, **k),
                   lambda **k: decode.sample_decode_ids_reference_algorithm(m, feats, None, **k),
                   lambda **k: m.sample_decode_ids([feats], None, **k), lambda **k: m.sample_decode([feats], None, **k),
                   lambda **k: evaluate.v2t_batch(m, [feats], None, sample=k)):
            with pytest.raises(ValueError):
                fn(**kw)
    with pytest.raises(ValueError, match="within the top-k candidates.*top_k"):
        decode.sample_decode_ids(m, feats, None, top_p=0.5)
    # sample= excludes beam_size and return_attn
    with pytest.raises(ValueError, match="excludes"):
        evaluate.v2t_batch(m, [feats], None, beam_size=3, sample=dict(num_samples=2))
    with pytest.raises(ValueError, match="excludes"):
        evaluate.v2t_batch(m, [feats], None, return_attn=True, sample=dict(num_samples=2))
    with pytest.raises(ValueError, match="excludes"):
        evaluate.v2t_single(m, [feats[0]], beam_size=2, sample={})
    with pytest.raises(ValueError):
        evaluate.v2t_single(m, [feats[0]], sample=dict(samples=2))


def test_seed_none_follows_torch_manual_seed():
    from vct_amd import decode
    torch.manual_seed(5)
    a = decode._draw_seed(None)
    torch.manual_seed(5)
    assert decode._draw_seed(None) == a and 0 <= a < 2 ** 31
    assert decode._draw_seed(12345) == 12345 and decode._draw_seed(2 ** 32 + 3) == 3


# ---- the C boundary --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from vct_amd import _lib
    return _lib.load()


def test_entry_point_validates_arguments(lib):
    from vct_amd import _lib, ops
    P = 4096                                 # never dereferenced: every check below returns before a launch

    def call(**kw):
        d = _lib.SampleSelectDesc()
        d.dtype, d.rows, d.V, d.t = _lib.BF16, 6, 100, 3
        d.x, d.ldx, d.out, d.out_stride, d.end_id, d.pad_id = P, 128, P, 30, END, PAD
        d.ended = d.ended_count = d.all_ended_at = d.step_logp = d.seq_logp = d.ctl = d.workspace = P
        d.workspace_bytes = 16                                           # the guard: a complete descriptor ends at VCT_E_WORKSPACE
        for k, v in kw.items():
            setattr(d, k, v)
        return lib.vct_sample_select(ctypes.byref(d), None)
    ARG, SHAPE, ALIGN, WS = -1, -2, -3, -4
    assert lib.vct_sample_select(None, None) == ARG
    assert call() == WS
    for name in ("x", "out", "ended", "ended_count", "all_ended_at", "step_logp", "seq_logp", "ctl", "workspace"):
        assert call(**{name: None}) == ARG, name
    assert call(dtype=7) == ARG and call(dtype=-1) == ARG
    assert call(rows=0) == SHAPE and call(V=0) == SHAPE and call(rows=-3) == SHAPE
    assert call(ldx=99) == SHAPE and call(ldx=100) == WS
    assert call(ctl=P + 4) == ALIGN and call(ctl=P + 8) == ALIGN and call(workspace=P + 8) == ALIGN
    need = lib.vct_sample_select_workspace_bytes(_lib.BF16, 6, 100)
    assert need == 6 * 1 * 130 * 4 == ops.sample_select_workspace_bytes(torch.bfloat16, 6, 100)
    assert call(workspace_bytes=need - 1) == WS
    for dt, tdt in ((_lib.BF16, torch.bfloat16), (_lib.F32, torch.float32)):
        for rows, V in ((1, 1), (130, 257), (80, 30522), (3, 2049)):
            assert lib.vct_sample_select_workspace_bytes(dt, rows, V) == ops.sample_select_workspace_bytes(tdt, rows, V)
    assert lib.vct_sample_select_workspace_bytes(_lib.F32, 80, 30522) == 80 * 30 * 130 * 4
    assert lib.vct_sample_select_workspace_bytes(7, 4, 10) == 0 and lib.vct_sample_select_workspace_bytes(0, 0, 10) == 0
    assert call(V=64 * 2048 + 1, ldx=1 << 20) == SHAPE                   # more chunks than the merging wave has lanes


def test_control_block_is_sixteen_bytes():
    """The device control block the engine fills by hand (its layout against the header: tests/test_abi_cpu.py)."""
    from vct_amd import _lib
    assert ctypes.sizeof(_lib.SampleCtl) == 16


def test_host_selection_of_the_reference_algorithm_is_the_restatement():
    """decode._sample_select_ref (torch float64, what sample_decode_ids_reference_algorithm selects with) against the numpy
    restatement on tied logits, with ended rows and every kind of setting."""
    from vct_amd import decode
    rng = np.random.default_rng(2)
    rows, V = 40, 300
    x = (rng.integers(-40, 40, (rows, V)) / 8.0).astype(np.float32)
    ended = np.arange(rows) % 3 == 1
    for k, p, temp in ((0, 1.0, 1.0), (1, 1.0, 2.0), (5, 0.9, 0.5), (64, 0.3, 1.0), (64, 1.0, 2.0)):
        it = np.float32(1.0 / temp)
        rt, rlp, _, margin, cut = S.select_step(x, ended, 31, 7, it, k, p, PAD, END)
        u = torch.tensor(decode.sample_uniforms(31, rows, 7), dtype=torch.float64)
        tok, lp, und = decode._sample_select_ref(torch.from_numpy(x), torch.from_numpy(ended), u, float(it), k, p, PAD, 1e-5)
        assert tok.tolist() == rt.tolist()
        np.testing.assert_allclose(lp.numpy(), rlp, rtol=0, atol=1e-12)
        assert und.tolist() == ((~ended) & ((margin <= 1e-5) | (cut <= 1e-5))).tolist()
