"""Caption quality metrics on integer ids: BLEU-1..4, ROUGE-L and CIDEr as coco-caption's Bleu(4), Rouge() and Cider() compute
them (the scorers behind the reference's COCOScorer, eval.py:42-123, whose sum gates its early stopping, train.py:248-270).
METEOR is absent: it needs a Java runtime and WordNet data.  `CaptionMetrics` is the host implementation in fp64;
`CaptionMetrics.to_device()` gives `DeviceCaptionMetrics`, which scores decoded id matrices where they are, on the GPU
(include/vct_hip.h: vct_capmetric_counts, vct_cider_d_eval, vct_capmetric_finish).

Definitions.  A candidate is cut BEFORE its first end token (dropped; a row without one is taken whole); references carry no
start or end token.  Per caption, with len the candidate's length and k = 1..4:
    guess_k = max(0, len - k + 1);   correct_k = sum over the candidate's distinct k-grams w of min(count_c(w), max_r count_r(w))
    reflen  = the reference length minimising (|len_r - len|, len_r)            ("closest"; a tie goes to the shorter reference)
    ROUGE-L: prec = max_r LCS_r / len, rec = max_r (LCS_r / len_r), F = (1 + beta^2) prec rec / (rec + beta^2 prec), 0 if either is 0
    CIDEr:   rewards.CiderD's formula (coco-caption's "CIDEr" is CIDEr-D: min-clipping, Gaussian length penalty, factor 10) with
             the document frequencies counted over the evaluated split's references.
Corpus level, from the integer sums over captions (tiny = 1e-15, small = 1e-9):
    p = 1;  for k = 1..4:  p *= (correct_k + tiny) / (guess_k + small),  Bleu_k = p ** (1 / k)
    ratio = (len + tiny) / (reflen + small);  if ratio < 1 every Bleu_k *= exp(1 - 1 / ratio)
    ROUGE_L = mean F,  CIDEr = mean per-caption CIDEr,  sum = Bleu_4 + ROUGE_L + CIDEr
A video without references gives an all-zero row and still counts in the means.  An empty candidate has zero counts, reflen =
the shortest reference, ROUGE 0 and CIDEr 0.  A candidate id outside [0, 2^31) matches nothing (all such ids are one unknown word).

Limits: no METEOR (the reference's early-stopping sum has four terms, this one three); `normalize_caption` approximates the
Stanford PTB tokenizer that coco-caption shells out to and does not reproduce it; the device path takes at most 64 tokens per
candidate."""
import math
import re
from collections import Counter
from typing import Dict, Hashable, List, Sequence

import numpy as np
import torch

from .rewards import CiderD, DeviceCiderD

COUNT_COLS = 12          # include/vct_hip.h: {len, reflen, correct_1..4, guess_1..4, lcs_max, 0}
KEYS = ("Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4", "ROUGE_L", "CIDEr", "sum")
_NO_END = -1             # an id no reference holds: CiderD must not cut references, the device cuts word-level rows at it
_UNKNOWN = -2            # what an id outside [0, 2^31) becomes (csrc/vct_capmetric.hip)

# coco-caption's tokenizer/ptbtokenizer.py removes these PTB tokens after tokenising
PUNCTUATIONS = ("''", "'", "``", "`", "-LRB-", "-RRB-", "-LCB-", "-RCB-", ".", "?", "!", ",", ":", "-", "--", "...", ";")
_SPLIT_OFF = re.compile(r"(\.\.\.|--|[.?!,:;\"(){}\[\]])")


def normalize_caption(s: str) -> List[str]:
    """A caption's words as the scorers see them: lower-cased, punctuation split off and removed (coco-caption's PUNCTUATIONS
    list, brackets and double quotes), split on whitespace; quotes around a word are stripped.  This APPROXIMATES the Stanford
    PTB tokenizer coco-caption runs and does not reproduce it: PTB splits contractions ("don't" -> "do", "n't"), this keeps
    them whole; numbers compared against a PTB-tokenised scorer can differ in the third digit on such captions."""
    out = []
    for w in _SPLIT_OFF.sub(" ", s.lower()).split():
        w = w.strip("'`")
        if w and w not in PUNCTUATIONS:
            out.append(w)
    return out


class WordTable:
    """Words -> ids, assigned in order of first appearance.  Build the references first; a candidate word never seen then gets
    a fresh id, which no reference holds, so it matches nothing (and the same unseen word keeps one id)."""

    def __init__(self):
        self.word2id: Dict[str, int] = {}

    def __len__(self):
        return len(self.word2id)

    def ids(self, words: Sequence[str]) -> List[int]:
        w2i = self.word2id
        return [w2i.setdefault(w, len(w2i)) for w in words]

    def encode(self, caption: str) -> List[int]:
        return self.ids(normalize_caption(caption))


def _grams(seq: Sequence[int], n: int = 4) -> Counter:
    return Counter(tuple(seq[i:i + k]) for k in range(1, n + 1) for i in range(len(seq) - k + 1))


def _lcs(cand: Sequence[int], ref: Sequence[int]) -> int:
    """Longest common subsequence by the bit-parallel row recurrence (one Python integer as the row word; the kernel's form)."""
    m = len(cand)
    if m == 0 or not ref:
        return 0
    where: Dict[int, int] = {}
    for j, t in enumerate(cand):
        where[t] = where.get(t, 0) | (1 << j)
    full = (1 << m) - 1
    v = full
    for t in ref:
        u = v & where.get(t, 0)
        v = ((v + u) | (v - u)) & full
    return m - bin(v).count("1")


def corpus_scores(counts, rouge_f, cider=None) -> dict:
    """The corpus-level numbers from per-caption rows: counts [C, >= 10] integers, rouge_f [C] and cider [C] (or None: CIDEr 0 and
    left out of the sum) -- the host statement of vct_capmetric_finish."""
    counts = np.asarray(counts)
    C = counts.shape[0]
    sums = [int(x) for x in counts[:, :10].astype(np.int64).sum(0)]
    tiny, small = 1e-15, 1e-9
    bleu, p = [], 1.0
    for k in range(4):
        p *= (sums[2 + k] + tiny) / (sums[6 + k] + small)
        bleu.append(p ** (1.0 / (k + 1)))
    ratio = (sums[0] + tiny) / (sums[1] + small)
    if ratio < 1.0:
        bp = math.exp(1.0 - 1.0 / ratio)
        bleu = [b * bp for b in bleu]
    rl = sum(float(x) for x in rouge_f) / C
    cd = sum(float(x) for x in cider) / C if cider is not None else 0.0
    out = {f"Bleu_{k + 1}": bleu[k] for k in range(4)}
    out.update(ROUGE_L=rl, CIDEr=cd, sum=bleu[3] + rl + cd)
    return out


class CaptionMetrics:
    """BLEU-1..4, ROUGE-L and CIDEr on ids, on the host in fp64 (module docstring).  refs: {video id: [id list, ...]}, ids in
    [0, 2^31), no start or end token.  n, sigma: CIDEr's n-gram orders and length-penalty width; beta: ROUGE-L's.  end_id: where
    a candidate is cut (None: candidates are taken whole)."""

    def __init__(self, refs: Dict[Hashable, List[Sequence[int]]], n: int = 4, sigma: float = 6.0, beta: float = 1.2, end_id=None):
        if not beta > 0:
            raise ValueError("CaptionMetrics: beta > 0")
        self.refs = {vid: [[int(t) for t in r] for r in rs] for vid, rs in refs.items()}
        for rs in self.refs.values():
            for r in rs:
                if r and (min(r) < 0 or max(r) > 0x7fffffff):
                    raise ValueError("CaptionMetrics: reference ids must be in [0, 2^31)")
        self.beta_sq = float(beta) * float(beta)
        self.end_id = None if end_id is None else int(end_id)
        self.cider = CiderD(self.refs, n=n, sigma=sigma, end_id=_NO_END)
        # per video: the clipping ceiling max_r count_r(w) of every 1..4-gram
        self._ceil = {}
        for vid, rs in self.refs.items():
            top: Dict[tuple, int] = {}
            for r in rs:
                for w, cnt in _grams(r).items():
                    if cnt > top.get(w, 0):
                        top[w] = cnt
            self._ceil[vid] = top

    def cut(self, cand: Sequence[int]) -> List[int]:
        out = []
        for t in cand:
            t = int(t)
            if t == self.end_id:
                break
            out.append(t if 0 <= t <= 0x7fffffff else _UNKNOWN)
        return out

    def _row(self, cand: Sequence[int], vid):
        rs = self.refs[vid]
        if not rs:
            return [0] * COUNT_COLS, (0.0, 0.0, 0.0), 0.0
        c = self.cut(cand)
        ln = len(c)
        reflen = min((abs(len(r) - ln), len(r)) for r in rs)[1]
        top = self._ceil[vid]
        correct = [0, 0, 0, 0]
        for w, cnt in _grams(c).items():
            correct[len(w) - 1] += min(cnt, top.get(w, 0))
        lcs = [_lcs(c, r) for r in rs]
        lcs_max = max(lcs)
        prec = lcs_max / ln if ln else 0.0
        rec = max((l / len(r) for l, r in zip(lcs, rs) if r), default=0.0)
        f = 0.0
        if prec != 0.0 and rec != 0.0:
            f = (1.0 + self.beta_sq) * prec * rec / (rec + self.beta_sq * prec)
        row = [ln, reflen] + correct + [max(0, ln - k) for k in range(4)] + [lcs_max, 0]
        return row, (prec, rec, f), self.cider.score(c, vid)

    def per_caption(self, cands: Dict[Hashable, Sequence[int]]) -> dict:
        """The per-caption rows, in cands' order: vids, counts int32 [C, 12], rouge fp64 [C, 3] = {prec, rec, F}, cider fp64 [C]."""
        vids = list(cands)
        if not vids:
            raise ValueError("CaptionMetrics: no candidates")
        rows = [self._row(cands[v], v) for v in vids]
        return dict(vids=vids, counts=np.asarray([r[0] for r in rows], np.int32).reshape(-1, COUNT_COLS),
                    rouge=np.asarray([r[1] for r in rows], np.float64).reshape(-1, 3), cider=np.asarray([r[2] for r in rows], np.float64))

    def score(self, cands: Dict[Hashable, Sequence[int]]) -> dict:
        """{Bleu_1..4, ROUGE_L, CIDEr, sum} of one candidate per video (KeyError for a video without a reference entry)."""
        pc = self.per_caption(cands)
        return corpus_scores(pc["counts"], pc["rouge"][:, 2], pc["cider"])

    def device_tables(self) -> dict:
        """Everything the three kernels read, as plain numpy arrays (no GPU needed): rewards.CiderD.device_tables() over the same
        references (vid_row and vid_ref_ptr are shared) plus the references' tokens as CSR, ref_tok_ptr int32 [R_total + 1] and
        ref_tok int32 [T_total] in vid_ref_ptr's reference order, beta_sq, and end_id = the candidates' end token (-1: none)."""
        t = self.cider.device_tables()
        ptr, toks = [0], []
        for rs in self.refs.values():
            for r in rs:
                toks += r
                ptr.append(len(toks))
        if len(toks) > 0x7fffffff:
            raise ValueError("CaptionMetrics.device_tables: more than 2^31 - 1 reference tokens")
        assert len(ptr) == int(t["vid_ref_ptr"][-1]) + 1 and list(t["vid_row"]) == list(self.refs)
        t.update(ref_tok_ptr=np.asarray(ptr, np.int32), ref_tok=np.asarray(toks, np.int32), beta_sq=self.beta_sq,
                 end_id=_NO_END if self.end_id is None else self.end_id)
        return t

    def to_device(self, device="cuda") -> "DeviceCaptionMetrics":
        """The same scores on the GPU: uploads device_tables() once; see DeviceCaptionMetrics."""
        return DeviceCaptionMetrics(self.device_tables(), device)


class DeviceCaptionMetrics:
    """CaptionMetrics on the device.  begin(capacity) starts an evaluation; add(ids, vids) scores one batch of decoded ids where
    they are (int64 [B, 1 + L] on the tables' device, any strides, column 0 = the start token, L <= 64; vids: B video ids) into
    device buffers -- enqueued on the current stream, no host synchronisation; result() folds the rows with one more launch,
    reads the eight doubles (the one synchronisation) and returns {Bleu_1..4, ROUGE_L, CIDEr, sum}.  An unknown video id raises
    KeyError and a wrong dtype / device / shape ValueError, both before any launch."""

    def __init__(self, tables: dict, device="cuda"):
        cd = DeviceCiderD(tables, device)
        self.device = cd.device
        self.n, self.sigma, self.end_id = cd.n, cd.sigma, int(tables["end_id"])
        self.log_nvid, self.two_sigma_sq, self.table_cap = cd.log_nvid, cd.two_sigma_sq, cd.table_cap
        self.beta_sq = float(tables["beta_sq"])
        self.vid_row, self.n_videos = cd.vid_row, cd.n_videos
        self.t = dict(cd.t)
        for k in ("ref_tok_ptr", "ref_tok"):
            a = tables[k] if tables[k].shape[0] else np.zeros(1, np.int32)      # (an empty table: the kernel still wants a pointer)
            self.t[k] = torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
        self._count = 0
        self._counts = self._rouge = self._cider = None

    def begin(self, capacity: int) -> "DeviceCaptionMetrics":
        """Start an evaluation of up to `capacity` captions (the buffers grow if more arrive)."""
        capacity = int(capacity)
        if capacity < 1:
            raise ValueError(f"DeviceCaptionMetrics.begin: capacity >= 1, got {capacity}")
        if self._counts is None or self._counts.shape[0] < capacity:
            self._alloc(capacity)
        self._count = 0
        return self

    def _alloc(self, capacity):
        old = (self._counts, self._rouge, self._cider)
        self._counts = torch.empty(capacity, COUNT_COLS, dtype=torch.int32, device=self.device)
        self._rouge = torch.empty(capacity, 3, dtype=torch.float64, device=self.device)
        self._cider = torch.empty(capacity, dtype=torch.float64, device=self.device)
        if self._count:
            for new, o in zip((self._counts, self._rouge, self._cider), old):
                new[:self._count].copy_(o[:self._count])

    def add(self, ids: torch.Tensor, vids) -> None:
        from . import ops
        if self._counts is None:
            raise RuntimeError("DeviceCaptionMetrics.add: call begin(capacity) first")
        ops.check_capmetric_ids(ids, self.device)
        if len(vids) != ids.shape[0]:
            raise ValueError(f"DeviceCaptionMetrics.add: ids [B, 1 + L] and B video ids, got {tuple(ids.shape)} and {len(vids)}")
        rows = torch.tensor([self.vid_row[v] for v in vids], dtype=torch.int32).to(self.device)      # KeyError: unknown video
        a, b = self._count, self._count + ids.shape[0]
        if b > self._counts.shape[0]:
            self._alloc(max(b, 2 * self._counts.shape[0]))
        ops.capmetric_counts(ids, rows, self, self._counts[a:b], self._rouge[a:b])
        ops.cider_d_eval(ids, rows, self, self._cider[a:b])
        self._count = b

    def rows(self):
        """The per-caption device rows added so far: (counts int32 [C, 12], rouge fp64 [C, 3], cider fp64 [C])."""
        c = self._count
        return self._counts[:c], self._rouge[:c], self._cider[:c]

    def result(self) -> dict:
        from . import ops
        if not self._count:
            raise ValueError("DeviceCaptionMetrics.result: nothing was added")
        out = ops.capmetric_finish(*self.rows()).tolist()
        return dict(zip(KEYS, out[:7]))

