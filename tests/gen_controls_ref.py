"""Numpy restatement of the generation controls (decode.GenerationControls; include/vct_hip.h, vct_logit_controls), written from
the stated semantics: plain Python loops over positions, the n-gram rule as "would h + [v] end in an n-gram that h already
contains", the beam history by explicit back-track.  Values are float32 arrays; a bf16 case holds bf16-exact float32 values and
rounds what it writes with round_bf16."""
import struct

import numpy as np


def f32(x):
    return struct.unpack("<f", struct.pack("<f", float(x)))[0]


def round_bf16(x):
    """float32 -> the nearest bf16 value (ties to even), as float32.  Finite values and infinities."""
    u = np.asarray(x, np.float32).reshape(-1).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def backtrack(tokens, parents, row, t):
    """The history h[0 .. t-1] of beam row `row` as of step t: tokens int [M, Lmax] (column s: the token appended at step s,
    column 0 the start token), parents int [Lmax, M] (row s: the parent ROW of every slot chosen at step s)."""
    h = [0] * t
    r = row
    for s in range(t - 1, 0, -1):
        h[s] = int(tokens[r, s])
        r = int(parents[s, r])
    h[0] = int(tokens[r, 0])
    return h


def ngram_banned(h, n):
    """The tokens v for which h + [v] would end in an n-gram that h already contains.  Only a token of h can complete one."""
    if n < 1 or len(h) + 1 < n:
        return set()
    grams = {tuple(h[i:i + n]) for i in range(len(h) - n + 1)}
    out = set()
    for v in sorted(set(h)):
        if tuple((h + [v])[-n:]) in grams:
            out.add(v)
    return out


def ban_set(h, end_id, min_length, n, banned_ids):
    t = len(h)
    out = set(int(b) for b in banned_ids)
    if t <= min_length:
        out.add(int(end_id))
    return out | ngram_banned(h, n)


def apply_row(x, h, end_id, min_length=0, n=0, theta=1.0, banned_ids=(), bf16=False):
    """One live row: x float32 [>= V] edited in place (every token named is < V)."""
    bans = ban_set(h, end_id, min_length, n, banned_ids)
    if theta != 1.0:
        th, inv = np.float32(f32(theta)), np.float32(f32(1.0 / theta))
        for v in sorted(set(h)):                     # once per distinct token
            if v in bans:
                continue
            y = x[v] * inv if x[v] > 0 else x[v] * th
            x[v] = round_bf16(y) if bf16 else y
    for v in bans:
        x[v] = -np.inf
    return x


def apply(x, hists, end_id, ended=None, bf16=False, **ctl):
    """x float32 [rows, ld] -> a processed copy; hists: one history (list) per row; ended: rows that are not touched."""
    out = np.array(x, np.float32, copy=True)
    for r, h in enumerate(hists):
        if ended is not None and ended[r]:
            continue
        apply_row(out[r], list(h), end_id, bf16=bf16, **ctl)
    return out


def apply_beam(x, tokens, parents, t, end_id, finished=None, bf16=False, **ctl):
    hists = [backtrack(tokens, parents, r, t) for r in range(x.shape[0])]
    return apply(x, hists, end_id, finished, bf16, **ctl)


def pack(min_length=0, n=0, theta=1.0, banned_ids=()):
    """The 160-byte control block, field by field."""
    raw = struct.pack("<i", min_length) + struct.pack("<i", n) + struct.pack("<f", theta) + struct.pack("<f", 1.0 / theta)
    raw += struct.pack("<i", len(banned_ids)) + b"\0" * 12
    for i in range(32):
        raw += struct.pack("<i", banned_ids[i] if i < len(banned_ids) else 0)
    return raw
