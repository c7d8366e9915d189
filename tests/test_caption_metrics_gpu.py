"""Caption metrics on the GPU: vct_capmetric_counts, vct_cider_d_eval and vct_capmetric_finish through ops against the independent
plain-Python reference tests/capmetric_ref.py (integers exact, prec / rec bit-equal, F within 1e-14), metrics.DeviceCaptionMetrics
against the host scorer, and evaluate.eval_metrics end to end on the toy dataset fixture."""
import json
import os

import numpy as np
import pytest
import torch

import capmetric_ref as R
from helpers import build_model, load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
START, END = 101, 102
NAN_BITS = 0x7FF8000000000000          # a quiet NaN's bit pattern read as int64: an id far outside [0, 2^31)
CANARY_I, CANARY_F = -123456789, -7.25
# F = (1 + b) * prec * rec / (rec + b * prec): three to five roundings with or without contraction, at most 2 ulp (4.4e-16), x 20
F_TOL = 1e-14
# device fp64 pow / exp a few ulp from the host's; sums of <= 300 terms in another order
FIN_REL, FIN_ABS = 1e-12, 1e-15


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _close(a, b, rel=FIN_REL, ab=FIN_ABS):
    return abs(a - b) <= rel * max(abs(a), abs(b)) + ab


def _scorer(refs, **kw):
    from vct_amd.metrics import CaptionMetrics
    cm = CaptionMetrics(refs, end_id=END, **kw)
    return cm, cm.to_device(DEV)


def _rows(dm, vids):
    return torch.tensor([dm.vid_row[v] for v in vids], dtype=torch.int32, device=DEV)


# ---- vct_capmetric_counts ------------------------------------------------------------------------------------------------------------
def _kernel_corpus():
    """Videos with 0, 1, 2, 5 and 33 references (33: more than the workgroup has waves) of lengths 1, 63, 64, 65 and 200 (longer
    than a wave), over a 2-word and a 12-word vocabulary."""
    rng = np.random.default_rng(11)

    def ref(n, vocab):
        return (5 + rng.integers(0, vocab, n)).tolist()
    refs = {
        "r0": [],
        "r1": [ref(1, 2)],
        "r2": [ref(63, 2), ref(64, 2)],
        "r33": [ref(n, 2) for n in [65, 200, 1, 64, 63] + rng.integers(1, 70, 28).tolist()],
        "r5": [ref(n, 12) for n in (65, 200, 10, 7, 12)],
        "r3": [ref(n, 12) for n in (5, 9, 14)],
    }
    assert len(refs["r33"]) == 33
    return refs, rng


def _candidates(refs, rng):
    """For every video: candidates of 0 (end token in column 1), 1, 3, 63 and 64 (no end token) tokens over both vocabularies,
    NaN-pattern / end-token / valid-word garbage behind the end token; then rows holding a negative and a >= 2^31 id."""
    L = 64
    rows, vids = [], []
    for vid in refs:
        for vocab in (2, 12):
            for n in (0, 1, 3, 63, 64):
                row = np.empty(1 + L, np.int64)
                row[0] = START
                row[1:1 + n] = 5 + rng.integers(0, vocab, n)
                if n < L:
                    row[1 + n] = END
                    tail = rng.choice(np.array([NAN_BITS, END, 5, 6, -1, 2 ** 40], np.int64), L - n - 1)
                    row[2 + n:] = tail
                rows.append(row)
                vids.append(vid)
    for vid in ("r2", "r5"):
        for bad in (-7, 2 ** 31, 2 ** 31 + 5, NAN_BITS):
            row = np.full(1 + L, END, np.int64)
            row[0] = START
            row[1:9] = [5, 6, bad, 5, bad, 6, 6, 5]
            rows.append(row)
            vids.append(vid)
    return np.stack(rows), vids


@pytest.fixture(scope="module")
def kernel_case():
    refs, rng = _kernel_corpus()
    ids, vids = _candidates(refs, rng)
    want = [R.caption_row(R.cut(row[1:], END), refs[v]) for row, v in zip(ids, vids)]
    cm, dm = _scorer(refs)
    return refs, ids, vids, want, cm, dm


def _check_counts(counts, rouge, want):
    counts, rouge = counts.cpu().numpy(), rouge.cpu().numpy()
    assert counts.tolist() == [w[0] for w in want]
    worst = 0.0
    for got, (_, (prec, rec, f)) in zip(rouge, want):
        assert got[0] == prec and got[1] == rec, (got, prec, rec)          # one correctly rounded division each
        err = abs(got[2] - f) / f if f else abs(got[2])
        worst = max(worst, err)
        assert err <= F_TOL and (f != 0.0 or got[2] == 0.0)
    return worst


def test_capmetric_counts_against_the_reference(kernel_case):
    from vct_amd import ops
    refs, ids, vids, want, cm, dm = kernel_case
    C = ids.shape[0]
    lens = {w[0][0] for w in want}
    assert {0, 1, 3, 63, 64} <= lens and any(w[0][10] == 64 for w in want)          # a full-word LCS: bit 63 and the carry out
    assert any(w[0][2] < w[0][6] and w[0][2] > 0 for w in want) and any(w[0][5] > 0 for w in want)
    dev_ids = torch.from_numpy(ids).to(DEV)
    rows = _rows(dm, vids)
    cbuf = torch.full((C + 2, 12), CANARY_I, dtype=torch.int32, device=DEV)
    rbuf = torch.full((C + 2, 3), CANARY_F, dtype=torch.float64, device=DEV)
    counts, rouge = ops.capmetric_counts(dev_ids, rows, dm, cbuf[1:C + 1], rbuf[1:C + 1])
    worst = _check_counts(counts, rouge, want)
    print(f"[capmetric_counts] {C} captions, worst F error {worst:.2e} (bound {F_TOL:.0e})")
    assert (cbuf[0] == CANARY_I).all() and (cbuf[C + 1] == CANARY_I).all()
    assert (rbuf[0] == CANARY_F).all() and (rbuf[C + 1] == CANARY_F).all()
    # a second call is bit-identical
    c2, r2 = ops.capmetric_counts(dev_ids, rows, dm)
    assert torch.equal(c2, counts) and r2.cpu().numpy().tobytes() == rouge.cpu().numpy().tobytes()


def test_capmetric_counts_strided_ids_and_short_tables(kernel_case):
    """A strided view (every other column of a wider matrix, rows reversed) gives the same rows; L = 0 (only the start column)
    is every caption empty."""
    from vct_amd import ops
    refs, ids, vids, want, _cm, dm = kernel_case
    C, W = ids.shape
    wide = torch.full((C, 2 * W + 3), END, dtype=torch.int64, device=DEV)
    wide[:, 1:1 + 2 * W:2] = torch.from_numpy(ids).to(DEV).flip(0)
    view = wide.flip(0)[:, 1:1 + 2 * W:2]
    assert view.stride(1) == 2 and not view.is_contiguous()
    counts, rouge = ops.capmetric_counts(view, _rows(dm, vids), dm)
    _check_counts(counts, rouge, want)
    only_start = torch.full((3, 1), START, dtype=torch.int64, device=DEV)
    counts, rouge = ops.capmetric_counts(only_start, _rows(dm, ["r0", "r2", "r33"]), dm)
    assert counts.cpu().tolist() == [R.caption_row([], refs[v])[0] for v in ("r0", "r2", "r33")]
    assert counts[1, 1] == 63 and counts[2, 1] == 1 and float(rouge.abs().sum()) == 0.0


# ---- vct_cider_d_eval ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def corpus64():
    refs, cands = R.random_corpus(7)
    refs = {v: [[t + 5 for t in r] for r in rs] for v, rs in refs.items()}
    cands = {v: [t + 5 for t in c] for v, c in cands.items()}
    L = 16
    ids = np.full((len(cands), 1 + L), END, np.int64)
    ids[:, 0] = START
    rng = np.random.default_rng(3)
    for i, c in enumerate(cands.values()):
        ids[i, 1:1 + len(c)] = c
        ids[i, 2 + len(c):] = rng.choice(np.array([NAN_BITS, 5, 6, 7], np.int64), L - len(c) - 1)       # garbage behind the end token
    cm, dm = _scorer(refs)
    return refs, cands, ids, cm, dm


def test_cider_d_eval_against_the_host(corpus64):
    from vct_amd import ops
    refs, cands, ids, cm, dm = corpus64
    vids = list(cands)
    C = len(vids)
    dev_ids = torch.from_numpy(ids).to(DEV)
    buf = torch.full((C + 2,), CANARY_F, dtype=torch.float64, device=DEV)
    got = ops.cider_d_eval(dev_ids, _rows(dm, vids), dm, buf[1:C + 1])
    host = cm.per_caption(cands)["cider"]
    ref = R.score(refs, cands)[3]
    g = got.cpu().numpy()
    assert (host > 0).sum() > C // 2
    for a, h, r in zip(g, host, ref):
        assert abs(a - h) <= 1e-12 * abs(h) and abs(a - r) <= 1e-12 * abs(r) and (h != 0.0 or a == 0.0)
    assert buf[0] == CANARY_F and buf[C + 1] == CANARY_F
    again = ops.cider_d_eval(dev_ids, _rows(dm, vids), dm)
    assert again.cpu().numpy().tobytes() == g.tobytes()


def test_cider_d_eval_rounds_to_cider_d_without_an_end_token(corpus64):
    """No end token in range: the two kernels see the same candidate, and the reward is the fp32 rounding of the score."""
    from vct_amd import ops
    refs, _cands, _ids, _cm, dm = corpus64
    rng = np.random.default_rng(5)
    vids = list(refs)
    for L in (1, 9, 64):
        ids = torch.from_numpy(5 + rng.integers(0, 12, (len(vids), 1 + L))).to(DEV)
        rows = _rows(dm, vids)
        score = ops.cider_d_eval(ids, rows, dm)
        reward = ops.cider_d(ids[:, None, :], rows, dm)
        assert torch.equal(score.float(), reward[:, 0]) and int((reward > 0).sum()) > len(vids) // 2


# ---- vct_capmetric_finish ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,longer", [(1, False), (1, True), (300, False), (300, True)])
def test_capmetric_finish_against_the_host_formula(C, longer):
    from vct_amd import ops
    rng = np.random.default_rng(C + longer)
    counts = np.zeros((C, 12), np.int32)
    counts[:, 0] = rng.integers(8, 20, C) if longer else rng.integers(3, 9, C)          # ratio >= 1 / < 1
    counts[:, 1] = rng.integers(8, 10, C) if longer else rng.integers(9, 15, C)
    for k in range(4):
        counts[:, 6 + k] = np.maximum(0, counts[:, 0] - k)
        counts[:, 2 + k] = rng.integers(0, counts[:, 6 + k] + 1) // (k + 1)
    counts[:, 10:] = rng.integers(0, 5, (C, 2))                                       # lcs_max and the pad column are not summed
    rouge = rng.random((C, 3))
    cider = rng.random(C) * 3
    want = R.corpus(counts.tolist(), rouge[:, 2].tolist(), cider.tolist())
    ratio = counts[:, 0].sum() / counts[:, 1].sum()
    assert (ratio >= 1) == longer
    d = [torch.from_numpy(a).to(DEV) for a in (counts, rouge, cider)]
    buf = torch.full((10,), CANARY_F, dtype=torch.float64, device=DEV)
    out = ops.capmetric_finish(d[0], d[1], d[2], buf[1:9])
    got = out.cpu().tolist()
    for i, k in enumerate(("Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4", "ROUGE_L", "CIDEr", "sum")):
        assert _close(got[i], want[k]), (k, got[i], want[k])
    assert got[7] == float(C) and buf[0] == CANARY_F and buf[9] == CANARY_F
    assert ops.capmetric_finish(*d).cpu().numpy().tobytes() == out.cpu().numpy().tobytes()
    # without CIDEr: slot 5 is 0 and the sum has two terms
    no = ops.capmetric_finish(d[0], d[1]).cpu().tolist()
    assert no[:5] == got[:5] and no[5] == 0.0 and no[6] == got[3] + got[4]


# ---- metrics.DeviceCaptionMetrics ----------------------------------------------------------------------------------------------------
def test_device_scorer_batches_and_host(corpus64):
    refs, cands, ids, cm, dm = corpus64
    vids = list(cands)
    dev_ids = torch.from_numpy(ids).to(DEV)
    dm.begin(len(vids))
    dm.add(dev_ids, vids)
    one = dm.result()
    rows_one = [t.clone() for t in dm.rows()]
    dm.begin(4)                                                     # a capacity too small: the buffers grow
    for a in range(0, len(vids), 7):
        dm.add(dev_ids[a:a + 7], vids[a:a + 7])
    seven = dm.result()
    assert seven == one and list(one) == ["Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4", "ROUGE_L", "CIDEr", "sum"]
    assert all(torch.equal(a, b) for a, b in zip(rows_one, dm.rows()))
    host = cm.score(cands)
    ref = R.score(refs, cands)[0]
    for k in host:
        assert _close(one[k], host[k], ab=0.0) and _close(one[k], ref[k], ab=0.0), (k, one[k], host[k], ref[k])
    assert torch.equal(rows_one[0].cpu(), torch.from_numpy(cm.per_caption(cands)["counts"]))


def test_device_scorer_refuses_before_any_launch(corpus64):
    from vct_amd.metrics import DeviceCaptionMetrics
    refs, cands, ids, cm, dm = corpus64
    vids = list(cands)
    dev_ids = torch.from_numpy(ids).to(DEV)
    fresh = DeviceCaptionMetrics(cm.device_tables(), DEV)
    with pytest.raises(RuntimeError, match="begin"):
        fresh.add(dev_ids[:2], vids[:2])
    fresh.begin(8)
    fresh._counts.fill_(CANARY_I)
    with pytest.raises(KeyError):
        fresh.add(dev_ids[:2], [vids[0], "no such video"])
    for bad in (dev_ids[:2].int(), dev_ids[:2].cpu(), dev_ids[:2][None], torch.zeros(2, 66, dtype=torch.int64, device=DEV),
                torch.zeros(0, 5, dtype=torch.int64, device=DEV), ids[:2]):
        with pytest.raises(ValueError):
            fresh.add(bad, vids[:2])
    with pytest.raises(ValueError):
        fresh.add(dev_ids[:3], vids[:2])
    with pytest.raises(ValueError, match="nothing"):
        fresh.result()
    assert fresh._count == 0 and bool((fresh._counts == CANARY_I).all())       # nothing was launched
    with pytest.raises(ValueError):
        fresh.begin(0)


# ---- evaluate.eval_metrics -----------------------------------------------------------------------------------------------------------
MC = {"modal": ["clip"], "modal_shape": [16], "text_enc_type": "CLIP", "embed_dim": 64, "dropout": 0.3, "loss_beta": 0.5,
      "matching": {"enable_tem": False, "matching_loss": "CSL"}, "activation": "gelu",
      "video_encoder": {"layer": 2, "nhead": 4, "feedforward": 128,
                        "mme": {"temporal": "encoding", "modal_different": True, "do_norm": False, "aggregation": "avg"}, "aoa": False},
      "caption_decoder": {"layer": 2, "nhead": 4, "feedforward": 128, "sce_loss_alpha": 0.5}, "pretrained_model": None}


@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    from test_data_cpu import ToyPrep, ToyTok, _dataset
    from vct_amd import data
    z = load_golden("dataloader.npz")
    meta = json.loads(str(z["meta"]))
    d = tmp_path_factory.mktemp("split_metrics")
    os.makedirs(d / "feats")
    for v in meta["vids"]:
        np.save(d / "feats" / f"{v}.npy", z[f"clip_{v}"])
    (d / "ann.json").write_text(json.dumps(meta["annotation"]))
    torch.manual_seed(5)
    m = build_model(MC, 2000, DEV, torch.float32)
    m.cap_preprocessor.tokenizer = ToyTok()
    ds = _dataset("msrvtt_val_by_video", d)
    dl = data.DeviceLoader(ds, 4, ToyPrep(), DEV, shuffle=False)
    return m, ds, dl


def _host_token(m, v2c, ids_by_vid):
    from vct_amd import evaluate
    from vct_amd.metrics import CaptionMetrics
    pre = m.cap_preprocessor
    refs = {v: [evaluate._reference_ids(pre, c) for c in caps] for v, caps in v2c.items()}
    return CaptionMetrics(refs, end_id=pre.end_id).score(ids_by_vid)


def _host_word(v2c, caps_by_vid):
    from vct_amd.metrics import CaptionMetrics, WordTable
    t = WordTable()
    refs = {v: [t.encode(c) for c in caps] for v, caps in v2c.items()}
    return CaptionMetrics(refs).score({v: t.encode(c) for v, c in caps_by_vid.items()})


def _same(a, b):
    return set(a) == set(b) and all(_close(a[k], b[k]) for k in a)


@pytest.mark.parametrize("beam", [None, 3])
def test_eval_metrics_end_to_end(toy, beam):
    from vct_amd import evaluate
    m, ds, dl = toy
    caps = evaluate.eval_epoch(m, dl, max_len=12, beam_size=beam)
    ids = {}
    for f, k, _c, vids in dl:
        ys = m.greedy_decode_ids(f, k, max_len=12) if beam is None else m.beam_decode_ids(f, k, beam_size=beam, max_len=12)
        ids.update(zip(vids, (r[1:] for r in ys.cpu().tolist())))
    # the dataset's own references
    tok, got_caps = evaluate.eval_metrics(m, dl, max_len=12, beam_size=beam, level="token", return_captions=True)
    assert got_caps == caps and list(got_caps) == list(caps)
    scored = [v for v in caps if v in ds.video2caption]               # the loader walks the directory; the split references fewer clips
    assert 0 < len(scored) <= len(caps)
    assert _same(tok, _host_token(m, ds.video2caption, {v: ids[v] for v in scored}))
    assert _same(evaluate.eval_metrics(m, dl, max_len=12, beam_size=beam, level="token"), tok)
    word = evaluate.eval_metrics(m, dl, max_len=12, beam_size=beam, level="word")
    assert _same(word, _host_word(ds.video2caption, {v: caps[v] for v in scored}))
    # references derived from the decoded captions themselves (an untrained model shares no word with the dataset's): each
    # video's caption minus its last word, and its neighbour's caption -- scores well away from 0 and 1; the scorer is reused
    vids = list(caps)
    v2c_ids = {v: [ids[v][:max(1, len(caps[v].split()) - 1)], ids[vids[(i + 1) % len(vids)]][:5]] for i, v in enumerate(vids)}
    v2c_str = {v: [" ".join(caps[v].split()[:-1]) + " .", caps[vids[(i + 1) % len(vids)]]] for i, v in enumerate(vids)}
    for level, v2c, host in (("token", v2c_ids, lambda: _host_token(m, v2c_ids, ids)), ("word", v2c_str, lambda: _host_word(v2c_str, caps))):
        scorer = evaluate.build_scorer(m, v2c, level)
        first = evaluate.eval_metrics(m, dl, max_len=12, beam_size=beam, level=level, scorer=scorer)
        assert evaluate.eval_metrics(m, dl, max_len=12, beam_size=beam, level=level, scorer=scorer) == first       # tables reused
        assert _same(first, host()) and first["ROUGE_L"] > 0.2 and first["Bleu_1"] > 0.2, (level, first)
        assert evaluate.metric_earlystop_score(first) == first["sum"]
    with pytest.raises(ValueError):
        evaluate.eval_metrics(m, dl, max_len=12, level="word", scorer=evaluate.build_scorer(m, v2c_ids, "token"))
    with pytest.raises(ValueError):
        evaluate.eval_metrics(m, dl, max_len=70)
