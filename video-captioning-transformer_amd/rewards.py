"""Sentence-level rewards and advantages for self-critical sequence training (trainer.CaptionTrainer.scst_step).  Host side, on
token ids: no device work, no tokenisation.  A caller may pass any `reward_fn(ids [B, N, L] int64 CPU, vids) -> float [B, N]`."""
import math
from collections import Counter
from typing import Dict, Hashable, List, Sequence

import numpy as np
import torch


def cut_sequence(row: Sequence[int], end_id: int) -> List[int]:
    """A caption's tokens as the reward sees them: cut after the first end token, which is KEPT (ending is rewarded); a row
    without an end token is taken whole.  The start token is the caller's to drop (CiderD drops column 0 of sampled ids)."""
    out = []
    for t in row:
        out.append(int(t))
        if int(t) == end_id:
            break
    return out


def _ngrams(seq: Sequence[int], n: int) -> Counter:
    c = Counter()
    for k in range(1, n + 1):
        for i in range(len(seq) - k + 1):
            c[tuple(seq[i:i + k])] += 1
    return c


class CiderD:
    """CIDEr-D on token ids.  refs: {video id: [token-id list, ...]} -- each reference WITHOUT a start token; it is cut after its
    first end token (kept) like a candidate.  For the n-gram orders k = 1..n:
        df(w)  = number of videos whose references contain n-gram w;   idf(w) = log(#videos) - log(max(1, df(w)))
        vector entry = count(w) * idf(w)
        sim_k(c, r) = sum_w min(c_w, r_w) * r_w / (|c| |r|)  (0 if either norm is 0), times exp(-(len(c) - len(r))^2 / (2 sigma^2))
        score = 10 * mean over k of mean over the video's references r of sim_k(c, r)
    A single-video corpus has idf = 0 everywhere and scores 0."""

    def __init__(self, refs: Dict[Hashable, List[Sequence[int]]], n: int = 4, sigma: float = 6.0, end_id: int = 102):
        if n < 1 or sigma <= 0:
            raise ValueError("CiderD: n >= 1 and sigma > 0")
        self.n, self.sigma, self.end_id = int(n), float(sigma), int(end_id)
        self.log_nvid = math.log(max(len(refs), 1))
        df = Counter()
        cooked = {}
        for vid, rs in refs.items():
            cs = [(len(s), _ngrams(s, self.n)) for s in (cut_sequence(r, self.end_id) for r in rs)]
            cooked[vid] = cs
            seen = set()
            for _, c in cs:
                seen.update(c)
            df.update(seen)
        self.df = df
        # per reference: (length, per-order {n-gram: tf-idf}, per-order norm)
        self.refs = {vid: [(ln,) + self._vec(c) for ln, c in cs] for vid, cs in cooked.items()}

    def _vec(self, counts: Counter):
        vec = [dict() for _ in range(self.n)]
        sq = [0.0] * self.n
        for w, tf in counts.items():
            v = tf * (self.log_nvid - math.log(max(1, self.df.get(w, 0))))
            vec[len(w) - 1][w] = v
            sq[len(w) - 1] += v * v
        return vec, [math.sqrt(x) for x in sq]

    def score(self, cand: Sequence[int], vid) -> float:
        """cand: token ids without the start token (cut here after its first end token)."""
        c = cut_sequence(cand, self.end_id)
        cvec, cnorm = self._vec(_ngrams(c, self.n))
        rs = self.refs[vid]
        if not rs:
            return 0.0
        total = 0.0
        for rlen, rvec, rnorm in rs:
            pen = math.exp(-float(len(c) - rlen) ** 2 / (2.0 * self.sigma ** 2))
            for k in range(self.n):
                if cnorm[k] == 0.0 or rnorm[k] == 0.0:
                    continue
                rv = rvec[k]
                s = 0.0
                for w, cw in cvec[k].items():
                    rw = rv.get(w)
                    if rw is not None:
                        s += min(cw, rw) * rw
                total += pen * s / (cnorm[k] * rnorm[k])
        return 10.0 * total / (self.n * len(rs))

    def __call__(self, ids, vids) -> np.ndarray:
        """ids int64 [B, N, L] on the CPU (column 0 = the start token, dropped); vids: B video ids.  Returns float32 [B, N]."""
        a = ids.numpy() if torch.is_tensor(ids) else np.asarray(ids)
        if a.ndim != 3 or len(vids) != a.shape[0]:
            raise ValueError(f"CiderD: ids [B, N, L] and B video ids, got {a.shape} and {len(vids)}")
        out = np.zeros(a.shape[:2], np.float32)
        for b, vid in enumerate(vids):
            for n in range(a.shape[1]):
                out[b, n] = self.score(a[b, n, 1:].tolist(), vid)
        return out


def advantages(r, baseline="mean_others") -> np.ndarray:
    """A[b, n] = r[b, n] - baseline.  "mean_others": the leave-one-out mean of the video's other samples (needs N >= 2; each
    video's advantages then sum to 0); an array [B]: a caller-supplied baseline per video (e.g. the greedy caption's reward).
    Returns float32 [B, N]."""
    r = np.asarray(r, np.float64)
    if r.ndim != 2:
        raise ValueError(f"advantages: rewards [B, N], got {r.shape}")
    B, N = r.shape
    if isinstance(baseline, str):
        if baseline != "mean_others":
            raise ValueError(f"advantages: unknown baseline {baseline!r}")
        if N < 2:
            raise ValueError("advantages: the leave-one-out baseline 'mean_others' needs num_samples >= 2")
        base = (r.sum(1, keepdims=True) - r) / (N - 1)
    else:
        base = np.asarray(baseline, np.float64)
        if base.shape != (B,):
            raise ValueError(f"advantages: a baseline array must be [B = {B}], got {base.shape}")
        base = base[:, None]
    return (r - base).astype(np.float32)
