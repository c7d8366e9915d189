"""fp64 restatement of text-video retrieval ranking for the tests of csrc/vct_retrieval.hip.  Plain numpy; it does not import
vct_amd.retrieval.

Definitions (text rows i, video columns j, gt[i] the video of text i):
  s = t^ v^T with L2-normalised rows;  plain: f = s;  dual softmax: f = s * p,  p = softmax over i of s[:, j] / tau.
  rank_t2v[i] = 1 + #{ j : f[i,j] > f[i,g] or (f[i,j] == f[i,g] and j < g) }
  rank_v2t[j] = the same count down column j for the best-scoring own text of video j (lowest index on ties); 0 without a text.

An fp32 kernel cannot be held to the fp64 ranks where two scores are closer than its rounding error, so every element also gets a
worst-case error band:
  plain:        band = band_s = (Dt + 8) * 2^-24            (Dt products and sums of values <= 1, the two norms, the two scalings)
  dual softmax: band = p (1 + |s| / tau) band_s + |f| (band_s / tau + 16 * 2^-24)
                (the error of s through s * exp(s / tau); the column statistic moves by at most band_s / tau; 16 ulp for exp / log).
A competitor whose |f - f_query| is within the sum of the two bands is AMBIGUOUS; every query gets the interval [lo, hi] of ranks
that the unambiguous competitors allow.  intervals() returns them; check() holds ranks and statistics against them."""
import numpy as np

EPS = 2.0 ** -24

# (Nv, per, Dt) of the GPU tests: the issue's six, then one below / at / one above the kernel's 128-video and 128-text tile extents
# (Nt = Nv * per - 3) and its 32-wide K tile
GPU_SHAPES = [(1, 1, 4), (2, 3, 4), (33, 2, 20), (67, 3, 20), (130, 5, 512), (257, 4, 1024),
              (127, 2, 20), (128, 2, 20), (129, 2, 20), (130, 1, 20), (131, 1, 20), (66, 2, 20),
              (33, 2, 28), (33, 2, 32), (33, 2, 36)]
GPU_MODES = [("plain", None), ("dual_softmax", 0.5), ("dual_softmax", 0.05)]


def case_seed(shape):
    return 1000 + 7 * shape[0] + shape[2]


def make_case(Nv, per, Dt, seed, shuffle=False):
    """The generator of the GPU tests: v standard normal, `per` texts per video minus 3 at the end (at least one text stays),
    t = v[gt] + lambda * noise, lambda log-uniform per text: lambda = c * sqrt(Dt / (2 ln Nv)) * 10^U(-0.3, 0), c = 1.4 below Dt = 512 and 1.2 from there.
    Why this range.  The own video scores ~1 / sqrt(1 + lambda^2) and the best of Nv others ~sqrt(2 ln Nv / Dt), so rank 1 is lost
    around lambda* = sqrt(Dt / (2 ln Nv)): a fixed 10^U(-1, 1) gives 51-63 % rank 1 at Dt = 20 but 81-99 % at Dt >= 512.  And the
    range must stay NEAR lambda*: a text far beyond it scores inside the bulk of the other videos' scores, where at Dt = 1024 the
    fp32 band (Dt + 8) 2^-24 almost always holds a competitor (measured: 10 % ambiguous queries with 10^U(-1, 1) sqrt(Dt / 20)),
    while a text just beyond it is beaten by a few tail scores only.  At Dt >= 512 about a tenth of the texts that lose rank 1
    are ambiguous, which leaves c little room (rank-1 share 0.78-0.79 at c = 1.2); at small Dt nothing is ambiguous and c = 1.4
    puts the share near 0.65."""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((Nv, Dt))
    gt = np.repeat(np.arange(Nv), per)
    gt = gt[:max(1, gt.size - 3)]
    if shuffle:
        gt = gt[rng.permutation(gt.size)]
    lam = (1.4 if Dt < 512 else 1.2) * np.sqrt(Dt / (2.0 * np.log(max(Nv, 2)))) * 10.0 ** rng.uniform(-0.3, 0.0, gt.size)
    t = v[gt] + lam[:, None] * rng.standard_normal((gt.size, Dt))
    return t.astype(np.float32), v.astype(np.float32), gt.astype(np.int32)


def exact_case(Nv, per, Dt, seed, nnz=(4, 16)):
    """Rows of 0 / +-1 with exactly 4 or 16 non-zeros: norms 2 and 4, every s a multiple of 1/16 and exact in fp32 -- many real ties."""
    rng = np.random.default_rng(seed)

    def rows(n):
        out = np.zeros((n, Dt), np.float32)
        for r in range(n):
            k = nnz[rng.integers(0, len(nnz))] if Dt >= 16 else 4
            at = rng.choice(min(Dt, 24), k, replace=False)        # a small support: overlaps, hence ties, are common
            out[r, at] = rng.choice([-1.0, 1.0], k)
        return out
    v = rows(Nv)
    gt = np.repeat(np.arange(Nv), per)
    gt = gt[:max(1, gt.size - 3)]
    gt = gt[rng.permutation(gt.size)].astype(np.int32)
    t = rows(gt.size)
    own = rng.random(gt.size) < 0.5                               # half of the texts ARE their video's row: score 1, tied with its copies
    t[own] = v[gt[own]]
    return t, v, gt


def scores(text, vid, mode="plain", tau=None):
    """(s, f, p) in fp64; p is None in plain mode."""
    t, v = np.asarray(text, np.float64), np.asarray(vid, np.float64)
    s = (t / np.sqrt((t * t).sum(1, keepdims=True))) @ (v / np.sqrt((v * v).sum(1, keepdims=True))).T
    if mode == "plain":
        return s, s, None
    assert mode == "dual_softmax" and tau is not None and tau > 0
    z = s / tau
    z = z - z.max(axis=0, keepdims=True)
    p = np.exp(z) / np.exp(z).sum(axis=0, keepdims=True)
    return s, s * p, p


def bands(s, f, p, Dt, mode="plain", tau=None):
    band_s = (Dt + 8) * EPS
    if mode == "plain":
        return np.full_like(s, band_s)
    return p * (1.0 + np.abs(s) / tau) * band_s + np.abs(f) * (band_s / tau + 16 * EPS)


def ranks_from_matrix(f, gt, strict=True):
    """The two rank vectors from a materialised matrix, by the definition above (strict=False: `>=` in place of `>`, the wrong
    rule a checker must reject).  A gt outside [0, Nv) gives rank 0."""
    f = np.asarray(f, np.float64)
    Nt, Nv = f.shape
    gt = np.asarray(gt, np.int64)
    rt, rv = np.zeros(Nt, np.int64), np.zeros(Nv, np.int64)
    jj, ii = np.arange(Nv), np.arange(Nt)
    for i in range(Nt):
        g = gt[i]
        if not 0 <= g < Nv:
            continue
        q = f[i, g]
        above = (f[i] >= q) if not strict else (f[i] > q) | ((f[i] == q) & (jj < g))
        rt[i] = 1 + np.count_nonzero(above)
    for j in range(Nv):
        own = np.flatnonzero(gt == j)
        if not own.size:
            continue
        col = f[:, j]
        b = own[np.argmax(col[own])]
        above = (col >= col[b]) if not strict else (col > col[b]) | ((col == col[b]) & (ii < b))
        rv[j] = 1 + np.count_nonzero(above)
    return rt, rv


def intervals(text, vid, gt, mode="plain", tau=None):
    """dict(rt, rv: the fp64 ranks; lo_t, hi_t, lo_v, hi_v: the rank intervals; amb_t, amb_v: the query has an ambiguous competitor)."""
    s, f, p = scores(text, vid, mode, tau)
    Nt, Nv = f.shape
    bd = bands(s, f, p, np.asarray(text).shape[1], mode, tau)
    gt = np.asarray(gt, np.int64)
    rt, rv = ranks_from_matrix(f, gt)
    lo_t, hi_t = np.zeros(Nt, np.int64), np.zeros(Nt, np.int64)
    lo_v, hi_v = np.zeros(Nv, np.int64), np.zeros(Nv, np.int64)
    for i in range(Nt):
        g = gt[i]
        if not 0 <= g < Nv:
            continue
        amb = np.abs(f[i] - f[i, g]) <= bd[i] + bd[i, g]
        amb[g] = False
        lo_t[i] = 1 + np.count_nonzero((f[i] > f[i, g]) & ~amb)
        hi_t[i] = lo_t[i] + np.count_nonzero(amb)
    for j in range(Nv):
        own = np.flatnonzero(gt == j)
        if not own.size:
            continue
        col, cb = f[:, j], bd[:, j]
        los, his = [], []
        for i in own:                                             # the video's rank is the best (smallest) rank of its own texts
            amb = np.abs(col - col[i]) <= cb + cb[i]
            amb[i] = False
            lo = 1 + np.count_nonzero((col > col[i]) & ~amb)
            los.append(lo)
            his.append(lo + np.count_nonzero(amb))
        lo_v[j], hi_v[j] = min(los), min(his)
    return dict(rt=rt, rv=rv, lo_t=lo_t, hi_t=hi_t, lo_v=lo_v, hi_v=hi_v, amb_t=hi_t > lo_t, amb_v=hi_v > lo_v)


def stats(ranks):
    """[R@1, R@5, R@10 as fractions, median, mean, n] of the non-zero ranks (the layout of one direction of the kernel's out[12])."""
    r = np.asarray(ranks, np.int64)
    r = r[r > 0]
    if not r.size:
        return [0.0] * 6
    return [np.count_nonzero(r <= k) / r.size for k in (1, 5, 10)] + [float(np.median(r)), float(r.sum()) / r.size, float(r.size)]


def check(ref, ranks_t2v, ranks_v2t, out12=None):
    """Violations (a list of strings, empty = pass) of the intervals by the given ranks and, when given, of the statistics'
    ranges by out12.  Where no query of a direction is ambiguous the intervals are points and this is an equality check."""
    bad = []
    for name, r, lo, hi in (("t2v", ranks_t2v, ref["lo_t"], ref["hi_t"]), ("v2t", ranks_v2t, ref["lo_v"], ref["hi_v"])):
        r = np.asarray(r, np.int64)
        if r.shape != lo.shape:
            bad.append(f"{name}: shape {r.shape} != {lo.shape}")
            continue
        out = np.flatnonzero((r < lo) | (r > hi))
        if out.size:
            k = out[0]
            bad.append(f"{name}: {out.size} ranks outside their interval, first query {k}: {r[k]} not in [{lo[k]}, {hi[k]}]")
    if out12 is not None:
        o = np.asarray(out12, np.float64)
        for d, (lo, hi) in enumerate(((ref["lo_t"], ref["hi_t"]), (ref["lo_v"], ref["hi_v"]))):
            best, worst, got = stats(lo), stats(hi), o[6 * d:6 * d + 6]
            for k in range(3):                                    # recalls fall as ranks grow
                if not worst[k] <= got[k] <= best[k]:
                    bad.append(f"dir {d} R@{(1, 5, 10)[k]}: {got[k]} not in [{worst[k]}, {best[k]}]")
            for k, what in ((3, "median"), (4, "mean")):
                if not best[k] <= got[k] <= worst[k]:
                    bad.append(f"dir {d} {what}: {got[k]} not in [{best[k]}, {worst[k]}]")
            if got[5] != best[5]:
                bad.append(f"dir {d} n: {got[5]} != {best[5]}")
    return bad
