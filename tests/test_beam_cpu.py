"""CPU-side checks of beam search: the numpy reference (tests/beam_ref.py) on the tiny decode weights, and the argument
checks of the two beam entry points (no device is touched)."""
import ctypes
import json

import numpy as np
import pytest

import beam_ref
import vct_oracle as O
from helpers import load_golden

START, END, PAD = 101, 102, 0


def _tiny():
    z = load_golden("tiny_decode.npz")
    mc = json.loads(str(z["model_config"]))
    cfg = O.cfg_from_model_config(mc, int(z["vocab"]))
    return z, cfg, O.init_params(cfg, seed=int(z["param_seed"]))


def _upto_first_end(row):
    hits = np.flatnonzero(row == END)
    return row[:hits[0] + 1] if hits.size else row


@pytest.mark.parametrize("tag", ["b1", "b3"])
def test_reference_beam_k1_is_greedy(tag):
    z, cfg, p = _tiny()
    feats = z[f"{tag}/feats"]
    ys = O.greedy_decode_ids(p, cfg, feats, None, max_len=12)
    ids, final, _ = beam_ref.beam_search(p, cfg, feats, None, 1, max_len=12)
    assert ids.shape == (feats.shape[0], 1, ys.shape[1])
    for b in range(feats.shape[0]):
        g = _upto_first_end(ys[b])
        assert np.array_equal(ids[b, 0, :g.size], g)


@pytest.mark.parametrize("K", [2, 3, 4])
def test_reference_beam_layout_and_scores(K):
    """Sorted final scores, [start, tokens, end, pad...] rows, and raw scores equal to the sum of the hypotheses' own
    log-probabilities under teacher forcing."""
    z, cfg, p = _tiny()
    feats = z["b3/feats"]
    B, L = feats.shape[0], 12
    ids, final, margin = beam_ref.beam_search(p, cfg, feats, None, K, max_len=L)
    assert ids.shape[:2] == (B, K) and 2 <= ids.shape[2] <= L
    assert margin > 0
    assert np.all(np.diff(final, axis=1) <= 0)
    assert np.all(ids[:, :, 0] == START)
    mem = O.mm_encoder_forward(p, cfg, feats, None)[0]
    for b in range(B):
        assert len({tuple(r) for r in ids[b]}) == K             # K distinct hypotheses
        for k in range(K):
            row = ids[b, k]
            hits = np.flatnonzero(row[1:] == END)
            n = hits[0] + 1 if hits.size else row.size - 1
            assert np.all(row[n + 1:] == PAD)
            raw = 0.0
            for t in range(1, n + 1):
                lg = O.decode_word(p, cfg, mem[b:b + 1], row[None, :t])[0].astype(np.float64)
                raw += lg[row[t]] - (lg.max() + np.log(np.exp(lg - lg.max()).sum()))
            assert abs(final[b, k] * n - raw) < 1e-4 * max(1.0, abs(raw))
    # the whole batch stops together: the matrix ends at max_len or right where the last beam finished
    if ids.shape[2] < L:
        ends = (ids[:, :, 1:] == END).any(2)
        assert ends.all()


def test_reference_selection_rules():
    """Tie to the smaller flat index, frozen finished slots, -inf slots of the first step."""
    K, V = 3, 7
    x = np.zeros((K, V), np.float32)
    x[0, [2, 5]] = 4.0                      # exact tie inside row 0: column 2 first
    x[1, 1] = 9.0
    s = np.array([0.0, -np.inf, -np.inf], np.float32)
    parent, tok, ns, nf, _ = beam_ref.select_step(x, s, np.zeros(K, bool), K, PAD, 5)
    assert parent.tolist() == [0, 0, 0] and tok.tolist() == [2, 5, 0]
    assert nf.tolist() == [False, True, False]
    s2 = np.array([-1.0, -2.0, -50.0], np.float32)
    parent, tok, ns2, nf2, _ = beam_ref.select_step(x, s2, np.array([True, False, False]), K, PAD, 5)
    assert parent[0] == 0 and tok[0] == PAD and ns2[0] == np.float32(-1.0) and nf2[0]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from vct_amd import _lib
    return _lib.load()


def test_beam_entry_points_validate_arguments(lib):
    P = ctypes.c_void_p(256)                # never dereferenced: every check below returns before a launch

    def sel(dtype=1, B=2, K=4, V=100, x=P, ldx=128, ws_bytes=1 << 20, pad=0, **kw):
        a = dict(scores=P, finished=P, parent=P, out=P, fc=P, at=P, ws=P)
        a.update(kw)
        return lib.vct_beam_select(dtype, B, K, V, x, ldx, a["scores"], a["finished"], a["parent"], a["out"], 30, END, pad,
                                   a["fc"], a["at"], 3, a["ws"], ws_bytes, None)

    assert sel(x=None) == -1
    assert sel(scores=None) == -1 and sel(parent=None) == -1 and sel(at=None) == -1 and sel(ws=None) == -1
    assert sel(dtype=7) == -1
    assert sel(K=0) == -2 and sel(K=17) == -2
    assert sel(K=8, V=5, ldx=5) == -2                   # K > V
    assert sel(ldx=99) == -2                            # ldx < V
    assert sel(B=0) == -2
    assert sel(pad=100) == -1                           # pad_id outside the vocabulary
    assert sel(ws_bytes=16) == -4

    def reo(dtype=1, L=2, M=8, Lmax=30, d=64, t=3, parent=P, src=P, dst=ctypes.c_void_p(512), stride=8 * 30 * 192):
        return lib.vct_beam_reorder(dtype, L, M, Lmax, d, t, parent, src, dst, stride, None)

    assert reo(parent=None) == -1 and reo(src=None) == -1 and reo(dst=None) == -1
    assert reo(dst=P) == -1                             # no in-place gather
    assert reo(t=0) == -2 and reo(t=31) == -2 and reo(M=0) == -2 and reo(L=0) == -2
    assert reo(stride=100) == -2                        # layers overlap
