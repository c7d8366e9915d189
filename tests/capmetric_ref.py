"""Plain-Python fp64 reference of the caption metrics (BLEU-4 "closest", ROUGE-L beta 1.2, CIDEr-D n = 4 sigma = 6), written from
the definitions in include/vct_hip.h / the metrics module's docstring with Counter n-grams and the textbook LCS table -- none
of the product's code, and not the bit-parallel recurrence."""
import math
from collections import Counter

TINY, SMALL = 1e-15, 1e-9


def cut(row, end_id):
    """Tokens of ids[1:] before the first end_id; ids outside [0, 2^31) become one unknown word."""
    out = []
    for t in row:
        t = int(t)
        if end_id is not None and t == end_id:
            break
        out.append(t if 0 <= t < 2 ** 31 else -2)
    return out


def ngrams(seq, k):
    return Counter(tuple(seq[i:i + k]) for i in range(len(seq) - k + 1))


def lcs_dp(a, b):
    prev = [0] * (len(b) + 1)
    for x in a:
        cur = [0]
        for j, y in enumerate(b):
            cur.append(prev[j] + 1 if x == y else max(prev[j + 1], cur[j]))
        prev = cur
    return prev[len(b)]


def caption_row(cand, refs, beta_sq=1.2 * 1.2):
    """cand: cut candidate; refs: list of token lists.  -> (12 integers, (prec, rec, F))."""
    if not refs:
        return [0] * 12, (0.0, 0.0, 0.0)
    ln = len(cand)
    reflen = sorted((abs(len(r) - ln), len(r)) for r in refs)[0][1]
    correct, guess = [], []
    for k in range(1, 5):
        c = ngrams(cand, k)
        rc = [ngrams(r, k) for r in refs]
        correct.append(sum(min(n, max(x[w] for x in rc)) for w, n in c.items()))
        guess.append(max(0, ln - k + 1))
    ls = [lcs_dp(cand, r) for r in refs]
    prec = max(ls) / ln if ln else 0.0
    rec = max([l / len(r) for l, r in zip(ls, refs) if len(r)] or [0.0])
    f = (1.0 + beta_sq) * prec * rec / (rec + beta_sq * prec) if prec != 0.0 and rec != 0.0 else 0.0
    return [ln, reflen] + correct + guess + [max(ls), 0], (prec, rec, f)


class Cider:
    """CIDEr-D over refs {vid: [token lists]}: df over videos, idf = log(#videos) - log(max(1, df))."""

    def __init__(self, refs, n=4, sigma=6.0):
        self.n, self.sigma, self.refs = n, sigma, refs
        self.lognv = math.log(max(len(refs), 1))
        self.df = Counter()
        for rs in refs.values():
            seen = set()
            for r in rs:
                for k in range(1, n + 1):
                    seen.update(ngrams(r, k))
            self.df.update(seen)

    def vec(self, seq, k):
        v = {w: tf * (self.lognv - math.log(max(1, self.df.get(w, 0)))) for w, tf in ngrams(seq, k).items()}
        return v, math.sqrt(sum(x * x for x in v.values()))

    def score(self, cand, vid):
        rs = self.refs[vid]
        if not rs:
            return 0.0
        total = 0.0
        for r in rs:
            pen = math.exp(-float(len(cand) - len(r)) ** 2 / (2.0 * self.sigma ** 2))
            for k in range(1, self.n + 1):
                cv, cn = self.vec(cand, k)
                rv, rn = self.vec(r, k)
                if cn == 0.0 or rn == 0.0:
                    continue
                total += pen * sum(min(x, rv[w]) * rv[w] for w, x in cv.items() if w in rv) / (cn * rn)
        return 10.0 * total / (self.n * len(rs))


def corpus(rows, fs, ciders=None):
    """rows: per-caption 12-integer lists; fs: per-caption F; ciders: per-caption CIDEr or None -> the reported dict."""
    C = len(rows)
    s = [sum(r[j] for r in rows) for j in range(10)]
    bleu, p = [], 1.0
    for k in range(4):
        p *= (s[2 + k] + TINY) / (s[6 + k] + SMALL)
        bleu.append(p ** (1.0 / (k + 1)))
    ratio = (s[0] + TINY) / (s[1] + SMALL)
    if ratio < 1:
        bleu = [b * math.exp(1 - 1 / ratio) for b in bleu]
    rl = math.fsum(fs) / C
    cd = math.fsum(ciders) / C if ciders is not None else 0.0
    out = {f"Bleu_{k + 1}": bleu[k] for k in range(4)}
    out.update(ROUGE_L=rl, CIDEr=cd, sum=bleu[3] + rl + cd)
    return out


def score(refs, cands, end_id=None):
    """refs {vid: [token lists]}, cands {vid: id list (no start token)} -> (dict, rows, rouge triples, ciders)."""
    cd = Cider(refs)
    rows, rouge, ciders = [], [], []
    for vid, c in cands.items():
        c = cut(c, end_id)
        row, tri = caption_row(c, refs[vid])
        rows.append(row)
        rouge.append(tri)
        ciders.append(cd.score(c, vid))
    return corpus(rows, [t[2] for t in rouge], ciders), rows, rouge, ciders


def random_corpus(seed, n_videos=64, vocab=12, max_refs=7, min_refs=1, len_lo=1, len_hi=14):
    """A seeded corpus with a small vocabulary (repeats and clipping are common): (refs, cands) with cands WITHOUT end token."""
    import random
    rng = random.Random(seed)
    refs, cands = {}, {}
    for v in range(n_videos):
        refs[f"v{v}"] = [[rng.randrange(vocab) for _ in range(rng.randint(len_lo, len_hi))]
                         for _ in range(rng.randint(min_refs, max_refs))]
        cands[f"v{v}"] = [rng.randrange(vocab) for _ in range(rng.randint(0 if v % 9 == 0 else 1, len_hi))]
    return refs, cands
