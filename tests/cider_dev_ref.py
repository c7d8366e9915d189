"""CIDEr-D from the device tables alone (rewards.CiderD.device_tables(), layout in include/vct_hip.h under vct_cider_d): a plain-loop
restatement of what the kernel does -- the key hash and the bounded linear probe in Python integers, the per-reference entries by
exact key comparison -- plus the corpora and candidate tables the CPU and GPU tests of the device reward share.  The scorer
reads nothing but the tables; the product package is imported by the tests, not here."""
import math

import numpy as np

END = 102
M32 = 0xffffffff


# ---- the tables, restated ----------------------------------------------------------------------------------------------------------
def key_of(gram):
    return tuple(int(t) for t in gram) + (-1,) * (4 - len(gram))


def key_hash(key):
    h = 0x811C9DC5
    for w in key:
        h = ((h ^ (w & M32)) * 0x01000193) & M32
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    h ^= h >> 16
    return h


def probe(T, key):
    """(found, idf, slot where the lookup ended, probes): linear probing from hash & (cap - 1), at most cap probes."""
    cap = T["table_cap"]
    keys = T["table_keys"]
    slot = key_hash(key) & (cap - 1)
    for i in range(cap):
        k = tuple(int(x) for x in keys[slot])
        if k[0] == -1:
            return False, T["log_nvid"], slot, i + 1
        if k == key:
            return True, float(T["table_idf"][slot]), slot, i + 1
        slot = (slot + 1) & (cap - 1)
    return False, T["log_nvid"], slot, cap


def score(T, cand, vid):
    """cand: token ids without the start token.  Reads only T."""
    n, end_id = T["n"], T["end_id"]
    c = []
    for t in cand:
        c.append(int(t))
        if int(t) == end_id:
            break
    uniq = [[] for _ in range(n)]          # per order: [key, tf] in first-occurrence order
    for k in range(1, n + 1):
        for i in range(len(c) - k + 1):
            key = key_of(c[i:i + k])
            for u in uniq[k - 1]:
                if u[0] == key:
                    u[1] += 1
                    break
            else:
                uniq[k - 1].append([key, 1])
    cvec, cnorm = [], []
    for k in range(n):
        v = [(key, tf * probe(T, key)[1]) for key, tf in uniq[k]]
        sq = 0.0
        for _, x in v:
            sq += x * x
        cvec.append(v)
        cnorm.append(math.sqrt(sq))
    row = T["vid_row"][vid]
    r0, r1 = int(T["vid_ref_ptr"][row]), int(T["vid_ref_ptr"][row + 1])
    if r1 == r0:
        return 0.0
    total = 0.0
    for r in range(r0, r1):
        e0, e1 = int(T["ref_ent_ptr"][r]), int(T["ref_ent_ptr"][r + 1])
        ents = {tuple(int(x) for x in T["ent_keys"][e]): float(T["ent_w"][e]) for e in range(e0, e1)}
        assert len(ents) == e1 - e0
        d = float(len(c) - int(T["ref_len"][r]))
        pen = math.exp(-(d * d) / T["two_sigma_sq"])
        for k in range(n):
            rn = float(T["ref_norm"][r, k])
            if cnorm[k] == 0.0 or rn == 0.0:
                continue
            s = 0.0
            for key, cw in cvec[k]:
                if key in ents:
                    s += min(cw, ents[key]) * ents[key]
            total += pen * s / (cnorm[k] * rn)
    return 10.0 * total / (n * (r1 - r0))


# ---- corpora -------------------------------------------------------------------------------------------------------------------------
SMALL_VOCAB = list(range(3, 11))          # 8 token ids (+ END): n-grams repeat, min(c, r) clips, tf > 1
SMALL_LENGTHS = (1, 4, 17, 64)


def small_corpus(seed=5):
    """6 videos with 0, 1, 2, 3, 4 and 4 references of 2 .. 7 tokens (end included); video 2 also holds the reference [END], video
    4 one of 71 tokens."""
    rng = np.random.default_rng(seed)

    def ref(ln):
        return [int(t) for t in rng.choice(SMALL_VOCAB, ln - 1)] + [END]
    refs = {v: [ref(int(rng.integers(2, 8))) for _ in range(cnt)] for v, cnt in enumerate((0, 1, 2, 3, 4, 4))}
    refs[2][1] = [END]
    refs[4][3] = ref(71)
    return refs


def small_candidates(refs, L, seed=9):
    """int64 [6, 5, 1 + L] (column 0 = start token 101).  Videos 0 .. 4: references of the video (video 0: random rows), cut to L
    columns, sample 0 unchanged, the others with a substitution or two.  Video 5: a row without an end token, an end token at
    the first position, one token repeated L times, ids the corpus does not hold, and a reference.  Behind every end token come
    corpus tokens, not pads: reading them would change the score."""
    rng = np.random.default_rng(seed + L)
    ids = np.zeros((6, 5, 1 + L), np.int64)
    ids[:, :, 0] = 101

    def put(b, s, toks):
        toks = list(toks)[:L]
        row = toks + [int(t) for t in rng.choice(SMALL_VOCAB, L - len(toks))]
        ids[b, s, 1:] = row

    for b in range(6):
        for s in range(5):
            rs = refs[b]
            if not rs:
                put(b, s, [int(t) for t in rng.choice(SMALL_VOCAB, int(rng.integers(1, 6)))] + [END])
                continue
            # (L = 1: the shortest references first, so that the [END] reference meets its equal)
            order = sorted(range(len(rs)), key=lambda i: len(rs[i])) if L == 1 else list(range(len(rs)))
            toks = list(rs[order[s % len(rs)]])
            for _ in range(0 if s == 0 else int(rng.integers(1, 3))):
                j = int(rng.integers(0, max(len(toks) - 1, 1)))
                if toks[j] != END:
                    toks[j] = int(rng.choice(SMALL_VOCAB))
            put(b, s, toks)
    put(5, 0, [int(t) for t in rng.choice(SMALL_VOCAB, L)])                  # no end token
    put(5, 1, [END])                                                          # end at the first position
    put(5, 2, [SMALL_VOCAB[2]] * L)                                           # tf = L, L - 1, L - 2, L - 3
    put(5, 3, [11, 12, 13, SMALL_VOCAB[0], 2000000000][:max(L - 1, 1)] + [END])   # n-grams the corpus does not hold
    put(5, 4, refs[5][1])
    return ids


def one_video_corpus():
    return {"only": [[3, 4, 5, END], [4, 4, 6, 7, END]]}


def large_corpus(videos=40, vocab=30522, seed=0, per_video=5):
    """tools/bench_scst.py's synthetic references."""
    rng = np.random.default_rng(seed)
    return {v: [[int(t) for t in rng.integers(1000, min(30000, vocab), int(rng.integers(6, 20)))] + [END] for _ in range(per_video)]
            for v in range(videos)}


def large_candidates(refs, L=29, seed=3):
    """int64 [videos, 5, 1 + L]: per video its references mutated -- unchanged, substitutions, a truncation (no end token), an early
    end, a mix of two references; pads (0) behind the end."""
    rng = np.random.default_rng(seed)
    V = len(refs)
    ids = np.zeros((V, 5, 1 + L), np.int64)
    ids[:, :, 0] = 101
    for b in range(V):
        rs = refs[b]
        rows = [list(rs[0])]
        sub = list(rs[1])
        for j in rng.choice(len(sub) - 1, 2, replace=False):
            sub[int(j)] = int(rng.integers(1000, 30000))
        rows.append(sub)
        rows.append(list(rs[2])[:int(rng.integers(2, len(rs[2]) - 1))])     # truncated: no end token, pads behind
        cut = int(rng.integers(1, len(rs[3]) - 1))
        rows.append(list(rs[3])[:cut] + [END] + list(rs[3])[cut:])            # an early end: the tail must not count
        rows.append(list(rs[4])[:3] + list(rs[0])[2:])
        for s, toks in enumerate(rows):
            toks = toks[:L]
            ids[b, s, 1:1 + len(toks)] = toks
    return ids
