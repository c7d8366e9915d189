"""Sentence-level rewards and advantages for self-critical sequence training (trainer.CaptionTrainer.scst_step).  Host side, on
token ids: no device work, no tokenisation.  A caller may pass any `reward_fn(ids [B, N, L] int64 CPU, vids) -> float [B, N]`.
CiderD.to_device() moves the same score onto the GPU (DeviceCiderD: ids stay on the device, rewards come back as a device tensor)."""
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


    # ---- the same score from flat tables (include/vct_hip.h, vct_cider_d) ---------------------------------------------------------
    def device_tables(self) -> dict:
        """Everything vct_cider_d reads, as plain numpy arrays (no GPU needed); layout and hash: include/vct_hip.h.
        The fp64 values are this object's own (idf by _vec's expression, tf * idf and the norms out of self.refs), so the kernel
        takes no logarithm.  Also: n, sigma, end_id, log_nvid, two_sigma_sq, table_cap and vid_row {video id: table row}.
        ValueError: n > 4 or a negative token id (a key is four int32 words, -1 is its padding)."""
        n = self.n
        if n > KEY_WORDS:
            raise ValueError(f"CiderD.device_tables: n-gram orders up to {KEY_WORDS}, got n = {n}")
        grams = list(self.df)
        for w in grams:
            if min(w) < 0 or max(w) > 0x7fffffff:
                raise ValueError(f"CiderD.device_tables: token ids must be in [0, 2^31), got {w}")
        cap = 2
        while cap < 2 * len(grams):
            cap *= 2
        table_keys = np.full((cap, KEY_WORDS), -1, np.int32)
        table_idf = np.zeros(cap, np.float64)
        if grams:
            keys = np.full((len(grams), KEY_WORDS), -1, np.int32)
            for i, w in enumerate(grams):
                keys[i, :len(w)] = w
            slots = (key_hash(keys) & np.uint32(cap - 1)).tolist()
            used = bytearray(cap)
            for i, w in enumerate(grams):
                s = slots[i]
                while used[s]:
                    s = (s + 1) & (cap - 1)
                used[s] = 1
                table_keys[s] = keys[i]
                table_idf[s] = self.log_nvid - math.log(max(1, self.df.get(w, 0)))
        vid_row, vid_ref_ptr, ref_len, ref_norm, ref_ent_ptr, ent_keys, ent_w = {}, [0], [], [], [0], [], []
        for vid, rs in self.refs.items():
            vid_row[vid] = len(vid_row)
            for ln, vec, norm in rs:
                ents = sorted((w + (-1,) * (KEY_WORDS - len(w)), v) for d in vec for w, v in d.items())
                ent_keys += [k for k, _ in ents]
                ent_w += [v for _, v in ents]
                ref_ent_ptr.append(len(ent_keys))
                ref_len.append(ln)
                ref_norm.append(list(norm) + [0.0] * (KEY_WORDS - n))
            vid_ref_ptr.append(len(ref_len))
        if len(ent_keys) > 0x7fffffff:
            raise ValueError("CiderD.device_tables: more than 2^31 - 1 reference n-grams")
        return dict(n=n, sigma=self.sigma, end_id=self.end_id, log_nvid=self.log_nvid, two_sigma_sq=2.0 * self.sigma ** 2,
                    table_cap=cap, table_keys=table_keys, table_idf=table_idf, vid_row=vid_row,
                    vid_ref_ptr=np.asarray(vid_ref_ptr, np.int32), ref_len=np.asarray(ref_len, np.int32),
                    ref_norm=np.asarray(ref_norm, np.float64).reshape(-1, KEY_WORDS), ref_ent_ptr=np.asarray(ref_ent_ptr, np.int32),
                    ent_keys=np.asarray(ent_keys, np.int32).reshape(-1, KEY_WORDS), ent_w=np.asarray(ent_w, np.float64))

    def to_device(self, device="cuda") -> "DeviceCiderD":
        """The same score as a device-side reward: uploads device_tables() once; see DeviceCiderD."""
        return DeviceCiderD(self.device_tables(), device)


KEY_WORDS = 4            # include/vct_hip.h, VCT_CIDER_MAX_ORDER: an n-gram key is four int32 words
DEVICE_MAX_LEN = 64      # VCT_CIDER_MAX_LEN: candidate tokens after the start column


def key_hash(keys) -> np.ndarray:
    """The corpus table's hash of n-gram keys [..., 4] int32 -> uint32 [...] (include/vct_hip.h: FNV-1a over the four words, then the
    murmur3 finaliser); the slot is hash & (table_cap - 1)."""
    k = np.asarray(keys, np.int32).astype(np.uint32).astype(np.uint64)
    m = np.uint64(0xffffffff)
    h = np.full(k.shape[:-1], 0x811C9DC5, np.uint64)
    for j in range(KEY_WORDS):
        h = ((h ^ k[..., j]) * np.uint64(0x01000193)) & m
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & m
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & m
    h ^= h >> np.uint64(16)
    return h.astype(np.uint32)


class DeviceCiderD:
    """CiderD on the device (ops.cider_d / vct_cider_d over CiderD.device_tables()).  __call__(ids, vids) -> fp32 DEVICE tensor
    [B, N]: ids int64 [B, N, L] on the tables' device (any strides; column 0 = the start token, L - 1 <= 64), vids: B video ids.
    Nothing is copied to the host and nothing waits for the device: the launch is enqueued on the current stream, behind whatever
    produced ids.  `on_device = True` is what CaptionTrainer.scst_step looks for.  An unknown video id raises KeyError before any
    device work; a video without references scores 0."""
    on_device = True

    def __init__(self, tables: dict, device="cuda"):
        self.device = torch.device(device)
        self.n, self.sigma, self.end_id = tables["n"], tables["sigma"], tables["end_id"]
        self.log_nvid, self.two_sigma_sq, self.table_cap = tables["log_nvid"], tables["two_sigma_sq"], tables["table_cap"]
        self.vid_row = tables["vid_row"]
        self.n_videos = len(self.vid_row)

        def up(name, min_rows=1):
            a = tables[name]
            if a.shape[0] < min_rows:              # (an empty table: the kernel still wants a pointer)
                a = np.zeros((min_rows,) + a.shape[1:], a.dtype)
            return torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
        self.t = {k: up(k) for k in ("table_keys", "table_idf", "vid_ref_ptr", "ref_len", "ref_norm", "ref_ent_ptr", "ent_keys", "ent_w")}
        self.device = self.t["table_keys"].device          # ("cuda" resolved to the device the tables went to)
        self._rows = {}

    def video_rows(self, vids) -> torch.Tensor:
        """int32 device tensor [B] of the videos' table rows (KeyError for an unknown id); the last few id lists are kept, so a
        caller may look them up ahead of the work the reward is queued behind."""
        key = tuple(vids)
        rows = self._rows.get(key)
        if rows is None:
            rows = torch.tensor([self.vid_row[v] for v in key], dtype=torch.int32).to(self.device)
            if len(self._rows) >= 8:
                self._rows.pop(next(iter(self._rows)))
            self._rows[key] = rows
        return rows

    def __call__(self, ids, vids, out=None) -> torch.Tensor:
        from . import ops
        if not torch.is_tensor(ids) or ids.dim() != 3 or len(vids) != ids.shape[0]:
            raise ValueError(f"DeviceCiderD: ids [B, N, L] and B video ids, got {getattr(ids, 'shape', type(ids))} and {len(vids)}")
        ops.check_cider_ids(ids, self.device)
        return ops.cider_d(ids, self.video_rows(vids), self, out)


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
