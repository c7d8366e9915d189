"""Text-video retrieval metrics of the matching head: recall at 1 / 5 / 10, median and mean rank for text->video and video->text
over a whole split (what the CLIP4Clip / MMT line of work reports).

Definitions (the host scorer below IS the definition; include/vct_hip.h states the same for the kernels):
  s[i, j] = t^_i . v^_j, rows L2-normalised without an epsilon (as the matching loss);
  mode "plain":         f = s (CSL's exp(temp) factor is monotone and dropped);
  mode "dual_softmax":  f[i, j] = s[i, j] * softmax_i(s[:, j] / tau)[i] (what CSL_WDS trains, without its factor B).
Ranks are 1-based and ties go to the lower index, as a stable descending sort gives:
  text->video, text i of video g = gt[i]:  1 + #{ j : f[i,j] > f[i,g] or (f[i,j] == f[i,g] and j < g) };
  video->text, video j with at least one text, i* its best-scoring own text (lowest index on ties):
                                           1 + #{ i : f[i,j] > f[i*,j] or (f[i,j] == f[i*,j] and i < i*) }
  (the best-ranked-own-caption convention of multi-sentence retrieval).
A video without a text, and a text whose gt is outside [0, n_videos), get rank 0 and enter no statistic.

`RetrievalMetrics` scores on the host in numpy fp64, materialising the matrix; `.to_device()` gives `DeviceRetrievalMetrics`,
which streams the matrix through csrc/vct_retrieval.hip and never stores it."""
from typing import Hashable, Optional, Sequence

import numpy as np
import torch

MODES = ("plain", "dual_softmax")
_STATS = ("R1", "R5", "R10", "MedianR", "MeanR", "n")


def _check_mode(mode, tau):
    if mode not in MODES:
        raise ValueError(f"retrieval mode {mode!r}: 'plain' or 'dual_softmax'")
    if mode == "dual_softmax":
        if tau is None or not float(tau) > 0.0:
            raise ValueError(f"retrieval mode 'dual_softmax' divides the similarity by tau: give tau > 0, got {tau!r}")
    elif tau is not None:
        raise ValueError("retrieval mode 'plain' takes no tau")


def rank_stats(ranks) -> dict:
    """{R1, R5, R10 in percent, MedianR, MeanR, n} of the non-zero ranks (rank 0 = not a query); all zero without one."""
    r = np.asarray(ranks, np.int64)
    r = r[r > 0]
    n = int(r.size)
    if n == 0:
        return dict(zip(_STATS, (0.0, 0.0, 0.0, 0.0, 0.0, 0)))
    rec = [100.0 * (float(np.count_nonzero(r <= k)) / float(n)) for k in (1, 5, 10)]
    return dict(zip(_STATS, rec + [float(np.median(r)), float(int(r.sum())) / float(n), n]))


def result_dict(t2v: dict, v2t: dict) -> dict:
    return {"t2v": t2v, "v2t": v2t, "rsum": sum(d[k] for d in (t2v, v2t) for k in ("R1", "R5", "R10"))}


class RetrievalMetrics:
    """The host scorer: numpy fp64 on the materialised [n_texts, n_videos] matrix."""

    def __init__(self, mode: str = "plain", tau: Optional[float] = None):
        _check_mode(mode, tau)
        self.mode, self.tau = mode, (float(tau) if tau is not None else None)

    def scores(self, text, vid) -> np.ndarray:
        t, v = np.asarray(text, np.float64), np.asarray(vid, np.float64)
        if t.ndim != 2 or v.ndim != 2 or t.shape[1] != v.shape[1] or not t.shape[0] or not v.shape[0]:
            raise ValueError(f"retrieval: text [Nt >= 1, Dt] and video [Nv >= 1, Dt] features expected, got {t.shape} and {v.shape}")
        s = (t / np.linalg.norm(t, axis=1, keepdims=True)) @ (v / np.linalg.norm(v, axis=1, keepdims=True)).T
        if self.mode == "plain":
            return s
        z = s / self.tau
        e = np.exp(z - z.max(axis=0, keepdims=True))
        return s * (e / e.sum(axis=0, keepdims=True))

    def ranks(self, text, vid, gt):
        """(ranks_t2v int64 [Nt], ranks_v2t int64 [Nv]); 0 where there is no query."""
        f = self.scores(text, vid)
        Nt, Nv = f.shape
        gt = np.asarray(gt, np.int64)
        if gt.shape != (Nt,):
            raise ValueError(f"retrieval: gt must be [{Nt}], got {gt.shape}")
        rt, rv = np.zeros(Nt, np.int64), np.zeros(Nv, np.int64)
        jj, ii = np.arange(Nv), np.arange(Nt)
        for i in range(Nt):
            g = gt[i]
            if 0 <= g < Nv:
                rt[i] = 1 + np.count_nonzero((f[i] > f[i, g]) | ((f[i] == f[i, g]) & (jj < g)))
        for j in range(Nv):
            own = np.flatnonzero(gt == j)
            if own.size:
                b = own[np.argmax(f[own, j])]            # (argmax: the first of equal maxima, own is ascending)
                rv[j] = 1 + np.count_nonzero((f[:, j] > f[b, j]) | ((f[:, j] == f[b, j]) & (ii < b)))
        return rt, rv

    def score(self, text, vid, gt) -> dict:
        """{"t2v": {R1, R5, R10, MedianR, MeanR, n}, "v2t": {...}, "rsum": the sum of the six recalls}; recalls in percent."""
        rt, rv = self.ranks(text, vid, gt)
        return result_dict(rank_stats(rt), rank_stats(rv))

    def to_device(self, device="cuda") -> "DeviceRetrievalMetrics":
        return DeviceRetrievalMetrics(self.mode, self.tau, device)


class DeviceRetrievalMetrics:
    """RetrievalMetrics on the device.  begin(n_videos, n_texts) preallocates the two embedding matrices and gt; add_videos(emb,
    vids) / add_texts(emb, vids) copy fp32 rows in where they are (device copies on the current stream, no synchronisation; the
    video name -> row map is a host dict, and a text may arrive before its video: rows are assigned on first sight of a name);
    result() enqueues the kernels, reads the twelve doubles (the one synchronisation) and returns RetrievalMetrics.score's dict.
    The per-query ranks of the last result() stay on the device as .ranks_t2v / .ranks_v2t.  tau: a float, or an fp32 device
    tensor [1] (a head's temperature) that is read on the device."""

    def __init__(self, mode: str = "plain", tau=None, device="cuda"):
        if torch.is_tensor(tau):
            if mode != "dual_softmax":
                raise ValueError("retrieval mode 'plain' takes no tau")
            if tau.dtype != torch.float32 or tau.numel() != 1:
                raise ValueError("retrieval: a tensor tau must be one fp32 element")
        else:
            _check_mode(mode, tau)
        if mode not in MODES:
            raise ValueError(f"retrieval mode {mode!r}: 'plain' or 'dual_softmax'")
        self.mode = mode
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"DeviceRetrievalMetrics runs on a GPU, got device {device!r}")
        self._tau = None
        if mode == "dual_softmax":
            self._tau = tau.detach().reshape(1).to(self.device) if torch.is_tensor(tau) else \
                torch.tensor([float(tau)], dtype=torch.float32, device=self.device)
        self._vid = self._text = self._gt = self._ws = None
        self._out = torch.empty(12, dtype=torch.float64, device=self.device)
        self.vid_row, self._have_v = {}, set()
        self._nt = self._cap_v = self._cap_t = 0
        self.ranks_t2v = self.ranks_v2t = None

    def begin(self, n_videos: int, n_texts: int) -> "DeviceRetrievalMetrics":
        n_videos, n_texts = int(n_videos), int(n_texts)
        if n_videos < 1 or n_texts < 1:
            raise ValueError(f"DeviceRetrievalMetrics.begin: n_videos >= 1 and n_texts >= 1, got {n_videos} and {n_texts}")
        self._cap_v, self._cap_t = n_videos, n_texts
        self._vid = self._text = None                     # allocated at the first add: the width comes with the rows
        self._gt = torch.empty(n_texts, dtype=torch.int32, device=self.device)
        self.vid_row = {}
        self._have_v = set()
        self._nt = 0
        self.ranks_t2v = self.ranks_v2t = None
        return self

    def _rows(self, emb, vids, what):
        if self._gt is None:
            raise RuntimeError(f"DeviceRetrievalMetrics.{what}: call begin(n_videos, n_texts) first")
        if not torch.is_tensor(emb) or emb.dtype != torch.float32 or emb.dim() != 2 or emb.device != self._gt.device:
            got = (tuple(emb.shape), emb.dtype, str(emb.device)) if torch.is_tensor(emb) else type(emb)
            raise ValueError(f"DeviceRetrievalMetrics.{what}: fp32 [B, Dt] on {self._gt.device} expected, got {got}")
        if len(vids) != emb.shape[0]:
            raise ValueError(f"DeviceRetrievalMetrics.{what}: {emb.shape[0]} rows and {len(vids)} video ids")
        Dt = emb.shape[1]
        if self._vid is None:
            if Dt % 4 or not 4 <= Dt <= 1024:
                raise ValueError(f"DeviceRetrievalMetrics.{what}: dimension {Dt}: the kernels take multiples of 4 up to 1024")
            self._vid = torch.empty(self._cap_v, Dt, dtype=torch.float32, device=self.device)
            self._text = torch.empty(self._cap_t, Dt, dtype=torch.float32, device=self.device)
        elif Dt != self._vid.shape[1]:
            raise ValueError(f"DeviceRetrievalMetrics.{what}: dimension {Dt}, earlier rows had {self._vid.shape[1]}")
        rows = []
        for v in vids:
            r = self.vid_row.get(v)
            if r is None:
                r = self.vid_row[v] = len(self.vid_row)
                if r >= self._cap_v:
                    raise ValueError(f"DeviceRetrievalMetrics.{what}: more than the {self._cap_v} videos begin() was told")
            rows.append(r)
        return rows

    def add_videos(self, emb: torch.Tensor, vids: Sequence[Hashable]) -> None:
        rows = self._rows(emb, vids, "add_videos")
        for v in vids:
            if v in self._have_v:
                raise ValueError(f"DeviceRetrievalMetrics.add_videos: video {v!r} was added twice")
            self._have_v.add(v)
        if rows == list(range(rows[0], rows[0] + len(rows))):
            self._vid[rows[0]:rows[0] + len(rows)].copy_(emb)
        else:
            self._vid.index_copy_(0, torch.tensor(rows, dtype=torch.long).to(self.device, non_blocking=True), emb)

    def add_texts(self, emb: torch.Tensor, vids: Sequence[Hashable]) -> None:
        """One row per caption; vids[k] is the video caption k belongs to."""
        rows = self._rows(emb, vids, "add_texts")
        a, b = self._nt, self._nt + len(rows)
        if b > self._cap_t:
            raise ValueError(f"DeviceRetrievalMetrics.add_texts: more than the {self._cap_t} texts begin() was told")
        self._text[a:b].copy_(emb)
        self._gt[a:b].copy_(torch.tensor(rows, dtype=torch.int32), non_blocking=True)
        self._nt = b

    def result(self) -> dict:
        from . import ops
        if self._vid is None or not self._nt or not self._have_v:
            raise ValueError("DeviceRetrievalMetrics.result: add videos and texts first")
        if len(self._have_v) != len(self.vid_row):
            missing = [v for v in self.vid_row if v not in self._have_v]
            raise ValueError(f"DeviceRetrievalMetrics.result: texts of {len(missing)} videos that were never added (first: {missing[0]!r})")
        nv, nt, Dt = len(self.vid_row), self._nt, self._vid.shape[1]
        need = ops.retrieval_workspace_bytes(nt, nv, Dt, self.mode)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        self.ranks_t2v = torch.empty(nt, dtype=torch.int32, device=self.device)
        self.ranks_v2t = torch.empty(nv, dtype=torch.int32, device=self.device)
        ops.retrieval_ranks(self._text[:nt], self._vid[:nv], self._gt[:nt], self.ranks_t2v, self.ranks_v2t, self._out, self._ws,
                            mode=self.mode, tau=self._tau)
        o = self._out.tolist()                                # the one synchronisation
        sides = []
        for d in (0, 6):
            r1, r5, r10, med, mean, n = o[d:d + 6]
            sides.append(dict(zip(_STATS, (100.0 * r1, 100.0 * r5, 100.0 * r10, med, mean, int(n)))))
        return result_dict(*sides)
