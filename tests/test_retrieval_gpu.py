"""Text-video retrieval evaluation on the GPU (csrc/vct_retrieval.hip through ops.retrieval_ranks, retrieval.DeviceRetrievalMetrics,
MMT4Caption.embed_videos, evaluate.eval_retrieval) against the fp64 restatement tests/retrieval_ref.py.

The kernels are fp32, the restatement fp64: a rank is held to the interval [lo, hi] that the restatement's worst-case error bands
allow (retrieval_ref: (Dt + 8) 2^-24 on s, and its propagation through the dual softmax), which is an equality wherever no
competitor is ambiguous -- tests/test_retrieval_cpu.py proves that this is the case for at least 97 % of the queries of every shape
used here.  Exact cases (0 / +-1 rows: every s exact in fp32) and the position-independence test are plain equalities."""
import functools

import numpy as np
import pytest
import torch

import retrieval_ref as R
from helpers import build_model, load_golden, model_config_of

pytestmark = pytest.mark.gpu
DEV = "cuda"
CANARY_I, CANARY_F = -123456789, -7.25


class Run:
    """One call of ops.retrieval_ranks with everything the kernels must not touch poisoned: NaN in the padding columns of the
    strided inputs and in the whole workspace, canaries around the three outputs and around the workspace."""

    def __init__(self, t, v, gt, mode, tau, pad_t=8, pad_v=12, phases=None):
        from vct_amd import ops
        Nt, Dt = t.shape
        Nv = v.shape[0]
        self.text = torch.full((Nt, Dt + pad_t), float("nan"), device=DEV)
        self.vid = torch.full((Nv, Dt + pad_v), float("nan"), device=DEV)
        self.text[:, :Dt] = torch.from_numpy(t).to(DEV)
        self.vid[:, :Dt] = torch.from_numpy(v).to(DEV)
        self.gt = torch.from_numpy(np.asarray(gt, np.int32)).to(DEV)
        self.rt = torch.full((Nt + 2,), CANARY_I, dtype=torch.int32, device=DEV)
        self.rv = torch.full((Nv + 2,), CANARY_I, dtype=torch.int32, device=DEV)
        self.out = torch.full((14,), CANARY_F, dtype=torch.float64, device=DEV)
        self.need = ops.retrieval_workspace_bytes(Nt, Nv, Dt, mode)
        self.ws = torch.full((self.need + 32,), 0xFF, dtype=torch.uint8, device=DEV)      # 0xFFFFFFFF: a NaN in every float
        self.tau = torch.tensor([tau], dtype=torch.float32, device=DEV) if tau is not None else None
        self.args = (self.text[:, :Dt], self.vid[:, :Dt], self.gt, self.rt[1:-1], self.rv[1:-1], self.out[1:13], self.ws[16:16 + self.need])
        self.kw = dict(mode=mode, tau=self.tau, phases=phases)
        self.call()

    def call(self):
        from vct_amd import ops
        ops.retrieval_ranks(*self.args, **self.kw)
        self.ranks_t, self.ranks_v = self.rt[1:-1].cpu().numpy().copy(), self.rv[1:-1].cpu().numpy().copy()
        self.stats = self.out[1:13].cpu().numpy().copy()
        assert self.rt[0] == CANARY_I and self.rt[-1] == CANARY_I and self.rv[0] == CANARY_I and self.rv[-1] == CANARY_I
        assert self.out[0] == CANARY_F and self.out[13] == CANARY_F
        assert bool((self.ws[:16] == 0xFF).all()) and bool((self.ws[16 + self.need:] == 0xFF).all())
        assert np.isfinite(self.stats).all()
        return self


@functools.lru_cache(maxsize=None)
def _case(shape, shuffle=False):
    return R.make_case(*shape, seed=R.case_seed(shape), shuffle=shuffle)


@functools.lru_cache(maxsize=None)
def _ref(shape, mode, tau, shuffle=False):
    t, v, gt = _case(shape, shuffle)
    return R.intervals(t, v, gt, mode, tau)


def _check(ref, run, tag):
    bad = R.check(ref, run.ranks_t, run.ranks_v, run.stats)
    assert not bad, (tag, bad)
    clear_t, clear_v = ~ref["amb_t"], ~ref["amb_v"]
    assert np.array_equal(run.ranks_t[clear_t], ref["rt"][clear_t]) and np.array_equal(run.ranks_v[clear_v], ref["rv"][clear_v]), tag
    if not ref["amb_t"].any() and not ref["amb_v"].any():
        want = np.asarray(R.stats(ref["rt"]) + R.stats(ref["rv"]))
        assert np.array_equal(run.stats, want), (tag, run.stats, want)


# ---- the kernels against the restatement -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,tau", R.GPU_MODES)
@pytest.mark.parametrize("shape", R.GPU_SHAPES)
def test_ranks_against_the_reference(shape, mode, tau):
    t, v, gt = _case(shape)
    ref = _ref(shape, mode, tau)
    run = Run(t, v, gt, mode, tau)
    _check(ref, run, (shape, mode, tau))
    first = (run.ranks_t.tobytes(), run.ranks_v.tobytes(), run.stats.tobytes())
    run.call()                                                        # a second call on the same inputs: the same bits
    assert first == (run.ranks_t.tobytes(), run.ranks_v.tobytes(), run.stats.tobytes())
    amb = int(ref["amb_t"].sum() + ref["amb_v"].sum())
    print(f"[retrieval] {shape} {mode} tau={tau}: {gt.size} x {shape[0]}, {amb} ambiguous queries, t2v R@1 {run.stats[0]:.3f}")


@pytest.mark.parametrize("mode,tau", R.GPU_MODES)
@pytest.mark.parametrize("shape", [(67, 3, 20), (130, 5, 512)])
def test_shuffled_texts_contiguous_inputs_and_bad_gt(shape, mode, tau):
    """Texts in shuffled order (a video's captions are scattered over the row tiles), contiguous inputs, and -- second call -- three
    ground truths outside the videos: rank 0, not counted, never used as an index."""
    t, v, gt = _case(shape, True)
    _check(_ref(shape, mode, tau, True), Run(t, v, gt, mode, tau, pad_t=0, pad_v=0), (shape, mode, tau, "shuffled"))
    bad = gt.copy()
    bad[[0, gt.size // 2, gt.size - 1]] = [-1, shape[0], 2 ** 31 - 1]
    run = Run(t, v, bad, mode, tau)
    ref = R.intervals(t, v, bad, mode, tau)
    _check(ref, run, (shape, mode, tau, "bad gt"))
    assert run.ranks_t[0] == 0 and run.ranks_t[-1] == 0 and run.stats[5] == gt.size - 3


# ---- exact cases: every s is exact in fp32, ties are real --------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(5, 3, 16), (150, 3, 32), (131, 2, 64), (300, 2, 24)])
def test_exact_cases_pin_the_tie_rule(shape):
    t, v, gt = R.exact_case(*shape, seed=shape[0])
    s = R.scores(t, v)[0]
    assert np.array_equal(s, np.round(s * 16) / 16)                   # multiples of 1 / 16: the generator's promise
    rt, rv = R.ranks_from_matrix(s, gt)
    ties = sum(int(np.count_nonzero(s[i] == s[i, gt[i]])) - 1 for i in range(gt.size))
    assert ties > (gt.size if shape[0] > 100 else 0)                  # the large cases: more than one tied competitor per query on average
    run = Run(t, v, gt, "plain", None)
    assert np.array_equal(run.ranks_t, rt) and np.array_equal(run.ranks_v, rv)
    assert np.array_equal(run.stats, np.asarray(R.stats(rt) + R.stats(rv)))
    # the dual softmax on the same rows: inside the intervals (an exact tie of s in one COLUMN stays a tie of f; across columns
    # the restatement marks it ambiguous)
    for tau in (0.5, 0.05):
        run = Run(t, v, gt, "dual_softmax", tau)
        assert not R.check(R.intervals(t, v, gt, "dual_softmax", tau), run.ranks_t, run.ranks_v, run.stats), (shape, tau)


# ---- position independence ------------------------------------------------------------------------------------------------------------
def test_ranks_do_not_depend_on_the_position_or_the_problem_around():
    """The first 40 texts of the first 20 videos (four zero columns appended: Dt = 24), alone and at the front of a larger problem
    (4 x 2 tiles) whose extra videos and texts live in those four columns only: they score exactly 0 against the sub-problem's rows,
    below every ground truth and every video's best own text.  No count changes, and because f[i, j] has the same bits in both
    problems the ranks are EQUAL, ambiguous queries included."""
    t, v, gt = _case((33, 2, 20))
    pad = lambda a, n: np.concatenate([a[:n], np.zeros((n, 4), np.float32)], axis=1)
    t, v, gt = pad(t, 40), pad(v, 20), gt[:40]
    assert gt.max() == 19
    rng = np.random.default_rng(9)
    extra = lambda n: np.concatenate([np.zeros((n, 20)), rng.standard_normal((n, 4))], axis=1).astype(np.float32)
    V, T = np.concatenate([v, extra(150)]), np.concatenate([t, extra(400)])
    G = np.concatenate([gt, 20 + rng.integers(0, 150, 400)]).astype(np.int32)
    s = R.scores(T, V)[0]
    own = np.asarray([s[:40][gt == j, j].max() for j in range(20)])
    assert (s[:40, 20:].max(1) < s[np.arange(40), gt] - 1e-3).all() and (s[40:, :20].max(0) < own - 1e-3).all()      # the premise
    small, big = Run(t, v, gt, "plain", None), Run(T, V, G, "plain", None)
    assert np.array_equal(big.ranks_t[:40], small.ranks_t) and np.array_equal(big.ranks_v[:20], small.ranks_v)
    assert (big.ranks_t > 0).all() and small.stats[5] == 40 and big.stats[5] == 440


# ---- against the matching head's own similarity kernel -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,tau", [("CSL", None), ("CSL_WDS", 0.5)])
def test_ranks_agree_with_the_head_similarity(kind, tau):
    from vct_amd.model.Matching import Matching
    B, Dt = 67, 20
    rng = np.random.default_rng(31)
    v = rng.standard_normal((B, Dt)).astype(np.float32)
    t = (v + 1.5 * rng.standard_normal((B, Dt))).astype(np.float32)
    gt = np.arange(B, dtype=np.int32)
    head = Matching((Dt, Dt), False, kind, tau, DEV)
    sim = head.similarity(torch.from_numpy(t).to(DEV), torch.from_numpy(v).to(DEV)).double().cpu()
    order_t, order_v = torch.argsort(-sim, dim=1, stable=True), torch.argsort(-sim, dim=0, stable=True)
    rt = np.asarray([int((order_t[i] == i).nonzero()[0, 0]) + 1 for i in range(B)])
    rv = np.asarray([int((order_v[:, j] == j).nonzero()[0, 0]) + 1 for j in range(B)])
    mode = "plain" if kind == "CSL" else "dual_softmax"
    run = Run(t, v, gt, mode, tau)
    ref = R.intervals(t, v, gt, mode, tau)
    assert not R.check(ref, run.ranks_t, run.ranks_v, run.stats)
    clear_t, clear_v = ~ref["amb_t"], ~ref["amb_v"]
    assert clear_t.sum() > 0.9 * B and clear_v.sum() > 0.9 * B
    assert np.array_equal(run.ranks_t[clear_t], rt[clear_t]) and np.array_equal(run.ranks_v[clear_v], rv[clear_v])
    assert 0.2 < np.mean(rt == 1) < 0.8


# ---- DeviceRetrievalMetrics ------------------------------------------------------------------------------------------------------------
def _exact_corpus(n_videos=37, per=3, Dt=32, seed=4):
    t, v, gt = R.exact_case(n_videos, per, Dt, seed)
    vids = [f"video{j}" for j in range(n_videos)]
    return t, v, gt, vids


def test_device_scorer_batches_orders_and_host():
    from vct_amd.retrieval import RetrievalMetrics
    t, v, gt, vids = _exact_corpus()
    host = RetrievalMetrics()
    want = host.score(t, v, gt)
    dm = host.to_device(DEV)
    dt, dv = torch.from_numpy(t).to(DEV), torch.from_numpy(v).to(DEV)
    dm.begin(len(vids), gt.size)
    dm.add_videos(dv, vids)
    dm.add_texts(dt, [vids[g] for g in gt])
    one = dm.result()
    assert one == want and list(one) == ["t2v", "v2t", "rsum"] and list(one["t2v"]) == ["R1", "R5", "R10", "MedianR", "MeanR", "n"]
    rt, rv = host.ranks(t, v, gt)
    assert np.array_equal(dm.ranks_t2v.cpu().numpy(), rt) and np.array_equal(dm.ranks_v2t.cpu().numpy(), rv)
    # batches, texts of a batch before its videos: rows are assigned on first sight, so the video ORDER differs -- the statistics
    # of a tie-free direction do not, and with ties the host scorer fed in the scorer's own row order agrees exactly
    dm.begin(len(vids), gt.size)
    order = np.argsort(gt, kind="stable")
    for a in range(0, gt.size, 10):
        idx = order[a:a + 10]
        dm.add_texts(dt[torch.from_numpy(idx).to(DEV)], [vids[g] for g in gt[idx]])
    for a in range(0, len(vids), 7):
        dm.add_videos(dv[a:a + 7], vids[a:a + 7])
    rows = np.asarray([dm.vid_row[x] for x in vids])
    v2 = np.empty_like(v)
    v2[rows] = v
    assert dm.result() == host.score(t[order], v2, rows[gt[order]])
    # refusals, before any launch
    with pytest.raises(ValueError):
        dm.begin(0, 5)
    dm.begin(2, 2)
    with pytest.raises(ValueError):
        dm.add_videos(dv[:2].double(), vids[:2])
    with pytest.raises(ValueError):
        dm.add_videos(dv[:2].cpu(), vids[:2])
    with pytest.raises(ValueError):
        dm.add_videos(dv[:3], vids[:2])
    with pytest.raises(ValueError, match="first"):
        dm.result()
    dm.add_videos(dv[:2], vids[:2])
    with pytest.raises(ValueError, match="twice"):
        dm.add_videos(dv[:1], vids[:1])
    with pytest.raises(ValueError, match="more than"):
        dm.add_texts(dt[:3], [vids[0]] * 3)
    dm.begin(2, 2)
    dm.add_videos(dv[:1], vids[:1])
    dm.add_texts(dt[:2], [vids[0], vids[1]])
    with pytest.raises(ValueError, match="never added"):
        dm.result()
    with pytest.raises(RuntimeError, match="begin"):
        RetrievalMetrics().to_device(DEV).add_videos(dv[:2], vids[:2])


# ---- MMT4Caption.embed_videos ------------------------------------------------------------------------------------------------------------
V = 131


def _match_model(name):
    import matching_ref as M
    z = load_golden(f"matching_{name}.npz")
    mc = model_config_of(z)
    m = build_model(mc, V, DEV, torch.float32, M.matching_params(mc, V, int(z["param_seed"])))
    n = len(mc["modal_shape"])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return z, m, [dev(z[f"feats{i}"]) for i in range(n)], [dev(z[f"mask{i}"]) for i in range(n)], dev(z["text_feats"])


@pytest.mark.parametrize("name", ["N", "L"])
def test_embed_videos_reproduces_the_head_similarity(name):
    """t^ . normalise(embed_videos(...)) against model.matching.similarity on the encoder's aggregation rows, to the 1e-5 that
    tests/test_matching_gpu.py holds this head's loss to.  'N': the no-temperature CSL head (the similarity IS the cosine);
    'L': a head with v_proj and a learned temperature (the similarity is the cosine times exp(temperature))."""
    z, m, feats, masks, text = _match_model(name)
    m.mode("match")
    m.eval()
    emb = m.embed_videos(feats, masks)
    assert emb.dtype == torch.float32 and tuple(emb.shape) == (text.shape[0], m.text_encoder.dim) and not emb.requires_grad
    _mem, _gmask, agg = m.video_encoder(feats, masks)
    sim = m.matching.similarity(text, agg.float().contiguous()).double()
    if m.matching.loss_fn.temperature is not None:
        sim = sim / torch.exp(m.matching.loss_fn.temperature.detach().double())
    unit = lambda a: a / a.norm(dim=1, keepdim=True)
    cos = unit(text.double()) @ unit(emb.double()).T
    err = float((cos - sim).abs().max())
    print(f"[embed_videos] {name}: max |cos - similarity| = {err:.2e}")
    assert err <= 1e-5
    assert torch.equal(m.embed_videos(feats, masks), emb)


def test_embed_videos_refuses_the_hierarchical_encoder():
    from hmm_ref import hmm_config, hmm_params
    mc = hmm_config([48, 24], [2, 1])
    hm = build_model(mc, V, DEV, torch.float32, hmm_params(mc, V, 5))
    feats = [torch.zeros(2, 5, 48, device=DEV), torch.zeros(2, 3, 24, device=DEV)]
    masks = [torch.zeros(2, 5, dtype=torch.bool, device=DEV), torch.zeros(2, 3, dtype=torch.bool, device=DEV)]
    with pytest.raises(NotImplementedError, match="hmme"):
        hm.embed_videos(feats, masks)


# ---- evaluate.eval_retrieval -------------------------------------------------------------------------------------------------------------
class _Split:
    """A by-video loader in memory: batches of (feats per modality, masks, captions, video ids) and the dataset's references."""

    def __init__(self, batches, video2caption):
        self.batches = batches
        self.dataset = type("D", (), {"video2caption": video2caption})()

    def __iter__(self):
        return iter(self.batches)


def _count_host_reads(monkeypatch):
    """Every way a value leaves the device in this code base, counted on CUDA tensors (tests/test_caption_metrics_gpu.py has no
    such counter to share, so this is the test's own)."""
    n = {"reads": 0}
    for name in ("tolist", "item", "cpu", "numpy", "__bool__", "__int__", "__float__", "__index__"):
        orig = getattr(torch.Tensor, name)

        def counted(self, *a, _orig=orig, **k):
            if self.is_cuda:
                n["reads"] += 1
            return _orig(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, name, counted)
    orig_to = torch.Tensor.to

    def counted_to(self, *a, **k):
        out = orig_to(self, *a, **k)
        if self.is_cuda and not out.is_cuda:
            n["reads"] += 1
        return out
    monkeypatch.setattr(torch.Tensor, "to", counted_to)
    for name in ("synchronize",):
        orig_sync = getattr(torch.cuda, name)

        def counted_sync(*a, _orig=orig_sync, **k):
            n["reads"] += 1
            return _orig(*a, **k)
        monkeypatch.setattr(torch.cuda, name, counted_sync)
    return n


@pytest.mark.parametrize("name", ["N", "W_fixed"])
def test_eval_retrieval_end_to_end(name, monkeypatch):
    """eval_retrieval over an in-memory split against the host scorer fed the same embeddings.  With the model's own video
    embeddings (real numbers; checked through the restatement's intervals) and with exact-case rows on both sides (the video rows
    through a stand-in for embed_videos): there the dicts are EQUAL.  One device->host read per evaluation."""
    from vct_amd import evaluate
    from vct_amd.retrieval import RetrievalMetrics
    z, m, feats, masks, _text = _match_model(name)
    m.mode("match")
    B, Dt = feats[0].shape[0], m.text_encoder.dim
    wds = name == "W_fixed"
    mode, tau = ("dual_softmax", 0.5) if wds else ("plain", None)
    # B videos in two batches, the first video also a second time under another name; 0..3 captions each; one id without an entry
    idx = list(range(B)) + [0]
    vids = [f"clip{k}" for k in range(len(idx))]
    et, ev, _g, _ = _exact_corpus(len(idx), 3, Dt, seed=8)
    caps_of = {vid: [f"{vid} caption {c}" for c in range(k % 4)] for k, vid in enumerate(vids)}
    del caps_of[vids[-2]]
    all_caps = [c for vid in vids for c in caps_of.get(vid, ())]
    row_of = {c: et[k] for k, c in enumerate(all_caps)}
    seen = []

    def text_feats_fn(captions, cap_vids):
        assert len(captions) == len(cap_vids) and all(c.startswith(v + " ") for c, v in zip(captions, cap_vids))
        seen.extend(captions)
        return torch.from_numpy(np.stack([row_of[c] for c in captions]))

    def batch(ks):
        sel = torch.tensor([idx[k] for k in ks], device=DEV)
        return [f[sel] for f in feats], [mk[sel] for mk in masks], None, [vids[k] for k in ks]
    half = len(idx) // 2
    split = _Split([batch(range(half)), batch(range(half, len(idx)))], caps_of)
    gt = np.asarray([vids.index(c.split(" ")[0]) for c in all_caps], np.int32)
    tx = np.stack([row_of[c] for c in all_caps])
    # 1. the model's own embeddings
    m.eval()
    emb = torch.cat([m.embed_videos(b[0], b[1]) for b in split.batches]).cpu().numpy()
    n = _count_host_reads(monkeypatch)
    got = evaluate.eval_retrieval(m, split, text_feats_fn=text_feats_fn)
    assert n["reads"] == 1, n
    monkeypatch.undo()
    assert seen == all_caps                                           # every reference caption of every video, once
    ref = R.intervals(tx, emb, gt, mode, tau)
    lo, hi = R.stats(ref["lo_t"]) + R.stats(ref["lo_v"]), R.stats(ref["hi_t"]) + R.stats(ref["hi_v"])
    for d, side in enumerate(("t2v", "v2t")):
        for k, key in enumerate(("R1", "R5", "R10")):
            assert 100 * hi[6 * d + k] - 1e-9 <= got[side][key] <= 100 * lo[6 * d + k] + 1e-9
        assert lo[6 * d + 4] <= got[side]["MeanR"] <= hi[6 * d + 4] and got[side]["n"] == int(lo[6 * d + 5])
    assert got["t2v"]["n"] == len(all_caps) and got["v2t"]["n"] == sum(1 for v_ in vids if caps_of.get(v_))
    assert evaluate.retrieval_earlystop_score(got) == got["rsum"]
    if not (ref["amb_t"].any() or ref["amb_v"].any()):
        assert got == RetrievalMetrics(mode, tau).score(tx, emb, gt)
    # 2. exact rows on both sides: equality with the host scorer
    row = {vid: ev[k] for k, vid in enumerate(vids)}

    def exact_embedder():                                             # a stand-in for embed_videos: the exact row of every video, batch by batch
        it = iter(split.batches)
        return lambda f, k: torch.from_numpy(np.stack([row[x] for x in next(it)[3]])).to(DEV)
    monkeypatch.setattr(m, "embed_videos", exact_embedder())
    got = evaluate.eval_retrieval(m, split, text_feats_fn=text_feats_fn)
    assert got == RetrievalMetrics(mode, tau).score(tx, ev, gt)
    # an explicit mode overrides the head's
    other = ("plain", None) if wds else ("dual_softmax", 0.05)
    monkeypatch.setattr(m, "embed_videos", exact_embedder())
    assert evaluate.eval_retrieval(m, split, text_feats_fn=text_feats_fn, mode=other[0], tau=other[1]) == \
        RetrievalMetrics(*other).score(tx, ev, gt)
    with pytest.raises(ValueError, match="video2caption"):
        evaluate.eval_retrieval(m, split.batches, text_feats_fn=text_feats_fn)


# ---- refusals through ops ----------------------------------------------------------------------------------------------------------------
def _ops_call(Nt=10, Nv=7, Dt=16, mode="plain", tau=None, ws_bytes=None):
    from vct_amd import ops
    need = ws_bytes if ws_bytes is not None else 1 << 16
    return ops.retrieval_ranks(torch.ones(Nt, Dt, device=DEV), torch.ones(Nv, Dt, device=DEV), torch.zeros(Nt, dtype=torch.int32, device=DEV),
                               torch.zeros(Nt, dtype=torch.int32, device=DEV), torch.zeros(Nv, dtype=torch.int32, device=DEV),
                               torch.zeros(12, dtype=torch.float64, device=DEV), torch.zeros(need, dtype=torch.uint8, device=DEV),
                               mode=mode, tau=tau)


def test_refusals_through_ops():
    from vct_amd import ops
    assert _ops_call()[5] == 10.0                                     # the call itself is fine
    with pytest.raises(ValueError, match="outside the kernels' range"):
        _ops_call(Dt=18)
    with pytest.raises(ValueError, match="outside the kernels' range"):
        _ops_call(Dt=1028)
    with pytest.raises(ValueError, match="outside the kernels' range"):
        _ops_call(Nv=0)
    with pytest.raises(ValueError, match="tau"):
        _ops_call(mode="dual_softmax")
    with pytest.raises(ValueError, match="VCT_E_WORKSPACE"):
        _ops_call(ws_bytes=ops.retrieval_workspace_bytes(10, 7, 16) - 16)
    with pytest.raises(ValueError, match="VCT_E_WORKSPACE"):
        _ops_call(mode="dual_softmax", tau=torch.ones(1, device=DEV), ws_bytes=ops.retrieval_workspace_bytes(10, 7, 16, "plain"))
