"""The self-critical reward on the GPU: vct_cider_d against rewards.CiderD, vct_scst_advantages against rewards.advantages, and
CaptionTrainer.scst_step / scst_epoch with a device reward against the host path.

Tolerance (derived): host and device both form the score in fp64 from bit-identical idf, r_w and reference norms (the tables
carry the host's own values); they differ in summation order and in the last bit of exp, about 1e-15 relative, and both round
once to fp32.  A device reward is therefore within ONE fp32 ulp of the host's: |dev - host| <= 2^-23 |host|, and exact zeros stay
exact zeros.  An advantage is within 2^-23 max|r| of its video's rewards.advantages value, the means likewise."""
import numpy as np
import pytest
import torch

import cider_dev_ref as D
from helpers import build_model, golden_params, load_golden, model_config_of, rel
import vct_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
CANARY = 12345.0
ULP = 2.0 ** -23


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from vct_amd import ops as _ops
    return _ops


def _cider(refs, **kw):
    from vct_amd.rewards import CiderD
    return CiderD(refs, end_id=D.END, **kw)


def _strided(ids_np):
    """The candidate table as a view with a gap behind every row and canaries (a corpus token) in it."""
    B, N, L = ids_np.shape
    full = torch.full((B, N + 1, L + 3), 5, dtype=torch.int64, device=DEV)
    view = full[:, :N, :L]
    view.copy_(torch.from_numpy(ids_np))
    assert not view.is_contiguous()
    return view


def _score_guarded(dev_fn, ids, vids):
    """Two calls into canary-guarded outputs: the guards stay, the two results agree bit for bit."""
    B, N = ids.shape[:2]
    outs = []
    for _ in range(2):
        full = torch.full((B + 2, N), CANARY, device=DEV)
        dev_fn(ids, vids, out=full[1:B + 1])
        torch.cuda.synchronize()
        assert bool((full[0] == CANARY).all()) and bool((full[-1] == CANARY).all())
        outs.append(full[1:B + 1].clone())
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    return outs[0].cpu().numpy()


def _assert_one_ulp(dev, host, what):
    err = np.abs(dev.astype(np.float64) - host.astype(np.float64))
    bound = ULP * np.abs(host.astype(np.float64))
    print(f"[cider] {what}: max |dev - host| / (2^-23 |host|) = {float((err / np.maximum(bound, 1e-300)).max()):.3g}, "
          f"{int((dev != host).sum())} of {host.size} differ, host > 0: {int((host > 0).sum())}")
    assert (err <= bound).all(), (what, float((err - bound).max()))
    assert (dev[host == 0] == 0).all()


# ---- 1. small vocabulary ---------------------------------------------------------------------------------------------------------
_SMALL = {}


def _small(n, sigma):
    if (n, sigma) not in _SMALL:
        refs = D.small_corpus()
        c = _cider(refs, n=n, sigma=sigma)
        _SMALL[(n, sigma)] = (refs, c, c.to_device(DEV))
    return _SMALL[(n, sigma)]


@pytest.mark.parametrize("sigma", [6.0, 0.5])
@pytest.mark.parametrize("n", [1, 2, 4])
@pytest.mark.parametrize("L", D.SMALL_LENGTHS)
def test_cider_d_small_vocabulary(ops, L, n, sigma):
    refs, host_fn, dev_fn = _small(n, sigma)
    ids_np = D.small_candidates(refs, L)
    vids = list(refs)
    host = host_fn(ids_np, vids)
    assert int((host[1:] > 0).sum()) * 2 >= host[1:].size          # the test cannot pass on zeros
    ids = _strided(ids_np)
    dev = _score_guarded(dev_fn, ids, vids)
    assert torch.equal(ids.cpu(), torch.from_numpy(ids_np))         # the candidates are read-only
    _assert_one_ulp(dev, host, f"small L={L} n={n} sigma={sigma}")
    assert (dev[0] == 0).all()                                      # the video without references
    if L == 64:
        # what follows an end token is never read into the score: other tokens behind it, the same bits
        ids2 = ids_np.copy()
        for b in range(6):
            for s in range(5):
                row = ids2[b, s, 1:]
                e = np.flatnonzero(row == D.END)
                if e.size:
                    row[e[0] + 1:] = 7
        assert (ids2 != ids_np).any()
        dev2 = _score_guarded(dev_fn, _strided(ids2), vids)
        assert np.array_equal(dev2.view(np.int32), dev.view(np.int32))


# ---- 2. a one-video corpus ---------------------------------------------------------------------------------------------------------
def test_cider_d_one_video_corpus_scores_zero(ops):
    c = _cider(D.one_video_corpus())
    ids_np = np.array([[[101, 3, 4, 5, D.END], [101, 4, 4, 6, 7], [101, D.END, 3, 3, 3]]], np.int64)
    host = c(ids_np, ["only"])
    dev = _score_guarded(c.to_device(DEV), _strided(ids_np), ["only"])
    assert (host == 0).all() and (dev == 0).all() and not np.signbit(dev).any()


# ---- 3. large vocabulary -----------------------------------------------------------------------------------------------------------
def test_cider_d_large_vocabulary(ops):
    refs = D.large_corpus()
    c = _cider(refs, n=4)
    ids_np = D.large_candidates(refs, L=29)
    vids = list(refs)
    host = c(ids_np, vids)
    assert host.shape == (40, 5) and int((host > 0).sum()) * 2 >= host.size
    dev = _score_guarded(c.to_device(DEV), _strided(ids_np), vids)
    _assert_one_ulp(dev, host, "large L=29 n=4")
    # the videos in another order, some twice: rows follow vids
    pick = [7, 7, 39, 0, 12]
    dev2 = _score_guarded(c.to_device(DEV), _strided(ids_np[pick]), pick)
    assert np.array_equal(dev2.view(np.int32), dev[pick].view(np.int32))


# ---- 4. vct_scst_advantages --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N", [(1, 2), (3, 5), (257, 5), (2, 64)])
@pytest.mark.parametrize("form", ["mean_others", "array"])
def test_scst_advantages(ops, B, N, form):
    from vct_amd.rewards import advantages
    rng = np.random.default_rng(100 * B + N)
    r = (rng.random((B, N)) * 3.0).astype(np.float32)
    r[0, 0] = 0.0
    base = (rng.random(B) * 3.0).astype(np.float32) if form == "array" else None
    want = advantages(r, "mean_others" if base is None else base)
    r64 = r.astype(np.float64)
    want_base = r64.mean(1) if base is None else base.astype(np.float64)          # the mean of a video's leave-one-out baselines
    want_means = (r64.mean(), want_base.mean())
    rmax = float(np.abs(r).max())
    outs = []
    for _ in range(2):
        full = torch.full((B * N + 2 + B + 2 + 4,), CANARY, device=DEV)
        adv, bo, means = full[1:1 + B * N], full[B * N + 3:B * N + 3 + B], full[B * N + B + 5:B * N + B + 7]
        rd = torch.from_numpy(r).to(DEV)
        got = ops.scst_advantages(rd, None if base is None else torch.from_numpy(base).to(DEV), adv=adv, base_out=bo, means=means)
        torch.cuda.synchronize()
        assert got[0].data_ptr() == adv.data_ptr() and torch.equal(rd.cpu(), torch.from_numpy(r))
        guards = [0, B * N + 1, B * N + 2, B * N + B + 3, B * N + B + 4, B * N + B + 7]
        assert all(float(full[g]) == CANARY for g in guards)
        outs.append(full.clone())
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    a = adv.cpu().numpy().reshape(B, N)
    err = float(np.abs(a.astype(np.float64) - want.astype(np.float64)).max())
    err_b = float(np.abs(bo.cpu().numpy().astype(np.float64) - want_base).max())
    m = means.cpu().numpy().astype(np.float64)
    print(f"[adv] B={B} N={N} {form}: adv err {err:.3g}, base err {err_b:.3g}, means err {abs(m[0] - want_means[0]):.3g} "
          f"{abs(m[1] - want_means[1]):.3g}, bound {ULP * rmax:.3g}")
    assert err <= ULP * rmax and err_b <= ULP * rmax
    assert abs(m[0] - want_means[0]) <= ULP * rmax and abs(m[1] - want_means[1]) <= ULP * rmax
    if base is None:
        assert np.abs(a.astype(np.float64).sum(1)).max() <= N * ULP * rmax      # a video's leave-one-out advantages sum to 0
    else:
        assert np.array_equal(bo.cpu().numpy(), base)
    # in place: the advantages may take the rewards' storage
    rd = torch.from_numpy(r).to(DEV)
    ops.scst_advantages(rd, None if base is None else torch.from_numpy(base).to(DEV), adv=rd.view(-1))
    assert torch.equal(rd.view(-1), adv)


def test_scst_advantages_refusals(ops):
    r = torch.zeros(3, 1, device=DEV)
    with pytest.raises(ValueError, match="num_samples >= 2"):
        ops.scst_advantages(r)
    ops.scst_advantages(r, torch.zeros(3, device=DEV))              # N = 1 with a baseline is fine
    with pytest.raises(ValueError):
        ops.scst_advantages(torch.zeros(3, 2, device=DEV, dtype=torch.float64))
    with pytest.raises(ValueError):
        ops.scst_advantages(torch.zeros(3, 2))
    with pytest.raises(ValueError):
        ops.scst_advantages(torch.zeros(3, 2, device=DEV), torch.zeros(2, device=DEV))


# ---- 5. scst_step with the reward on the device --------------------------------------------------------------------------------------
def _tiny():
    z = load_golden("tiny_train.npz")
    mc = model_config_of(z)
    V = int(z["vocab"])
    cfg = O.cfg_from_model_config(mc, V)
    return z, mc, V, golden_params(z, cfg)


def _fresh(mc, V, p):
    from vct_amd.trainer import CaptionTrainer, FusedAdam
    m = build_model(mc, V, DEV, torch.float32, p)
    m.train()
    return m, CaptionTrainer(m, FusedAdam(m, lr=1e-4))


def _refs_from_samples(ids0, V, seed=1):
    """References the samples can score against: per video two of its own sampled captions, one of them with substitutions, and
    one caption of the next video."""
    from vct_amd.rewards import cut_sequence
    rng = np.random.default_rng(seed)
    a = ids0.cpu().numpy()
    B = a.shape[0]
    refs = {}
    for b in range(B):
        r0 = cut_sequence(a[b, 0, 1:].tolist(), D.END)
        r1 = cut_sequence(a[b, 1, 1:].tolist(), D.END)
        for j in range(0, max(len(r1) - 1, 0), 3):
            r1[j] = int(rng.integers(103, V))
        r2 = cut_sequence(a[(b + 1) % B, 2, 1:].tolist(), D.END)
        refs[f"v{b}"] = [r0, r1, r2]
    return refs


@pytest.mark.parametrize("baseline", ["mean_others", "greedy"])
def test_scst_step_device_reward_matches_the_host_path(ops, baseline):
    z, mc, V, p = _tiny()
    feats, mask = torch.from_numpy(z["feats"]).to(DEV), torch.from_numpy(z["mask"]).to(DEV)
    B, N, kw = feats.shape[0], 4, dict(num_samples=4, max_len=10, seed=7, baseline=baseline)
    m, tr = _fresh(mc, V, p)
    ids0 = m.sample_decode_ids(feats, mask, num_samples=4, max_len=10, seed=7)
    host_fn = _cider(_refs_from_samples(ids0, V))
    vids = [f"v{b}" for b in range(B)]
    r0 = host_fn(ids0.cpu(), vids)
    assert r0.max() > r0.min() and (r0 > 0).sum() * 2 >= r0.size
    out_h = tr.scst_step(feats, mask, host_fn, vids, **kw)
    gh = m.flat_grads.clone()
    m2, tr2 = _fresh(mc, V, p)
    calls = []
    orig = ops.scst_advantages
    ops.scst_advantages = lambda *a, **k: calls.append("adv") or orig(*a, **k)
    try:
        out_d = tr2.scst_step(feats, mask, host_fn.to_device(DEV), vids, **kw)
    finally:
        ops.scst_advantages = orig
    assert calls == ["adv"]
    assert torch.equal(out_h["ids"], ids0) and torch.equal(out_d["ids"], ids0)
    for k in ("reward_mean", "baseline_mean"):
        assert isinstance(out_h[k], float)
        assert torch.is_tensor(out_d[k]) and out_d[k].dim() == 0 and out_d[k].is_cuda and out_d[k].dtype == torch.float32
    lh, ld = float(out_h["loss"]), float(out_d["loss"])
    rmax = float(np.abs(r0).max())
    eg = rel(m2.flat_grads, gh)
    print(f"[scst_step device] {baseline}: loss {ld:.7g} host {lh:.7g}, grads rel {eg:.3g}, reward_mean {float(out_d['reward_mean']):.9g} "
          f"host {out_h['reward_mean']:.9g}, baseline_mean {float(out_d['baseline_mean']):.9g} host {out_h['baseline_mean']:.9g}, "
          f"bound {ULP * rmax:.3g}")
    assert abs(ld - lh) <= 1e-5 * abs(lh)
    assert float(gh.abs().sum()) > 0 and eg < 1e-3
    assert abs(float(out_d["reward_mean"]) - out_h["reward_mean"]) <= ULP * rmax
    assert abs(float(out_d["baseline_mean"]) - out_h["baseline_mean"]) <= ULP * rmax


class _Loader:
    def __init__(self, batches):
        self.batches = batches

    def __iter__(self):
        return iter(self.batches)


def test_scst_epoch_device_reward_matches_the_host_path(ops):
    from vct_amd.trainer import FusedAdam, scst_epoch
    z, mc, V, p = _tiny()
    feats, mask = torch.from_numpy(z["feats"]), torch.from_numpy(z["mask"])
    B = feats.shape[0]
    m, _ = _fresh(mc, V, p)
    ids0 = m.sample_decode_ids(feats.to(DEV), mask.to(DEV), num_samples=4, max_len=10, seed=7)
    host_fn = _cider(_refs_from_samples(ids0, V))
    vids = [f"v{b}" for b in range(B)]
    batches = [([feats], [mask], None, vids), ([feats.flip(0)], [mask.flip(0)], None, vids[::-1])]
    kw = dict(num_samples=4, max_len=10, seed=7)
    res, seen = [], []

    def recording(ids, v):                       # the host path, and the largest reward of the epoch for the bound
        r = host_fn(ids, v)
        seen.append(float(np.abs(r).max()))
        return r
    for fn in (recording, host_fn.to_device(DEV)):
        m, _ = _fresh(mc, V, p)
        res.append(scst_epoch(m, FusedAdam(m, lr=1e-4), _Loader(batches), fn, **kw))
    (lh, rh), (ld, rd) = res
    print(f"[scst_epoch device] loss {ld:.7g} host {lh:.7g}; reward {rd:.9g} host {rh:.9g}")
    assert isinstance(ld, float) and isinstance(rd, float) and rh > 0
    assert abs(ld - lh) <= 1e-5 * abs(lh)
    assert len(seen) == 2 and abs(rd - rh) <= ULP * max(seen)


# ---- 6. refusals before any launch ---------------------------------------------------------------------------------------------------
def test_device_reward_refusals(ops, monkeypatch):
    from vct_amd import _lib
    from vct_amd.trainer import CaptionTrainer, FusedAdam
    refs = D.small_corpus()
    dev_fn = _cider(refs).to_device(DEV)
    assert dev_fn.on_device is True
    launched = []
    lib = _lib.load()
    monkeypatch.setattr(_lib, "load", lambda: launched.append(1) or lib)      # every launch goes through _lib.load()
    vids = list(refs)
    good = torch.from_numpy(D.small_candidates(refs, 4)).to(DEV)
    with pytest.raises(ValueError, match="int64"):
        dev_fn(good.int(), vids)
    with pytest.raises(ValueError, match="device"):
        dev_fn(good.cpu(), vids)
    with pytest.raises(ValueError, match="64"):
        dev_fn(torch.zeros(6, 5, 66, dtype=torch.int64, device=DEV), vids)
    with pytest.raises(KeyError):
        dev_fn(good, vids[:5] + ["no such video"])
    with pytest.raises(ValueError):
        dev_fn(good, vids[:5])
    # the step: a recorded executor, an active exchange and a 66-column sample are refused before the sampler runs
    z, mc, V, p = _tiny()
    feats, mask = torch.from_numpy(z["feats"]).to(DEV), torch.from_numpy(z["mask"]).to(DEV)
    m = build_model(mc, V, DEV, torch.float32, p)
    m.train()
    monkeypatch.setattr(m, "sample_decode_ids", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the step must refuse before it samples")))

    class ActiveExchange:
        active, world, group = True, 2, None
    opt = torch.optim.Adam([m.flat_params], lr=1e-4)
    for kw in (dict(use_graph=True), dict(launch_list=True), dict(exchange=ActiveExchange())):
        with pytest.raises(NotImplementedError, match="eager|single-process"):
            CaptionTrainer(m, opt, **kw).scst_step(feats, mask, dev_fn, num_samples=2)
    tr = CaptionTrainer(m, opt)
    with pytest.raises(ValueError, match="max_len"):
        tr.scst_step(feats, mask, dev_fn, list(refs)[:feats.shape[0]], num_samples=2, max_len=66)
    with pytest.raises(KeyError):
        tr.scst_step(feats, mask, dev_fn, ["nobody"] * feats.shape[0], num_samples=2)
    assert not launched
