"""fp64 references, per-element bounds, checkers, shapes and a fault-injecting float32 emulation of the kernels between the data loader
and the first encoder layer: the three encoder front ends (csrc/vct_enc_frontend_ex.hip, csrc/vct_mm_frontend.hip, vct_enc_frontend_* in
csrc/vct_elem.hip), the hierarchical encoder's row routing (csrc/vct_hmm_mix.hip) and the data movers vct_gather_pad_rows, vct_cast and
vct_transpose (csrc/vct_elem.hip).  Shared by tests/test_frontend_ref_cpu.py (which checks THIS file against torch autograd, max-pool
backward, torch's own bf16 rounding and oracle/vct_oracle.py, and shows that every checker rejects the seeded faults) and
tests/test_frontend_kernels_gpu.py.  Plain torch / numpy in float64 on the CPU; nothing here reads the library.

Operations (include/vct_hip.h; written from the formulas, not from the kernels' code paths).  Stream i of n owns the memory rows
off_i .. off_i + T_i (off_i = sum_{j<i} (T_j + 1), S = off_n), its aggregation row first.  All act on the operands as stored.
    add_rows   add[s] = temporal(s) + modal(s): temporal = temp[s] (fixed) or emb_w[tidx[s]] (learned), modal = modal_w[labels[s]]; a term
               whose index lies outside its table is absent (zero), and so is the modal term of a single stream
    front_fwd  pre[b, off_i] = add[off_i] + mean_t | max_t u_i[b, t];  pre[b, off_i+1+t] = add[off_i+1+t] + u_i[b, t];
               key_pad[b, off_i] = 0, key_pad[b, off_i+1+t] = mask_i[b, t];  arg_i[b, c] = the FIRST t that holds max_t u_i[b, t, c]
    norm_fwd   x0 = LayerNorm(pre) * mask (row_ref.ln_fwd on pre; the dropout comes after the norm), mean / rstd stored
    norm_bwd   dpre = LayerNorm backward of dx * mask from the saved statistics (exact operands); param_ws[b * n + i] = (dgamma, dbeta)
               summed over the T_i + 1 rows of (b, i)
    front_bwd  du_i[b, t] = dpre[b, off_i+1+t] + share: dpre[b, off_i] / T_i (avg), or dpre[b, off_i] where t == arg_i[b, c] and 0
               elsewhere (max);  d_modal[l] = sum over b and the s with labels[s] == l of dpre[b, s];  d_emb[e] likewise over tidx[s] == e,
               exact +0 in the rows nobody reads;  rows with an index outside the table enter neither sum
    mix_fwd    x[b, s] = take[s] ? y[b, s] : x0[b, s]
    mix_bwd    dy = take ? dx : +0;  acc = (take ? 0 : float(dx)) with init, acc += float(dx) on the restarting rows without it (one
               IEEE fp32 addition: restated in float32, bit for bit);  closing form dx0 = round(acc + float(dx))
    gather_pad out[b, t] = store[offsets[idx[b]] + t] for t < len(clip idx[b]) else +0;  mask[b, t] = 1 where padded
    cast_rne   fp32 bit pattern -> bf16 bit pattern, round to nearest even, in integer arithmetic: NaN -> a quiet NaN of the same sign;
               else (x + 0x7FFF + bit 16 of x) >> 16 (the carry out of the mantissa runs into the exponent, 0x7F7F8000 and above reach
               infinity, denormals are rounded like any other value: nothing is flushed)
    transpose  dst[c, r] = src[r, c] on 16-bit patterns

Bounds.  Every bound is  u_out |ref| + e  as in tests/row_ref.py: u_out = 2^-24 (fp32 result) or 2^-8 (bf16), u = 2^-24, e the
first-order propagation of one relative u per fp32 operation.  The only fp32 operations are additions, one division and exact
selections; none of the bounds is sized from a kernel's output and nothing here is a measured allowance.
    add        u |add| where both terms exist, 0 where one is absent (x + 0 is exact)
    frame row  e_add + u |pre|
    avg row    the sum of T terms in any order: T u sum_t |u_t| / T on the mean; the division: u |mean|; the addition: e_add + u |pre|
    max row    the selection is exact: e_add + u |pre|
    du         avg: 2 u |g0 / T| (vct_enc_frontend_bwd multiplies by a rounded 1 / T, the others divide: both granted) + u |du|;
               max: u |du| (the placement is judged exactly: check_placement);  behind the norm both carry dpre's own errors
    d_modal,   K u sum |terms| with K = B * cnt terms in any order, plus the terms' own errors behind the norm;  integer-valued dx: the sums
    d_emb      are exact in any order and must match bit for bit
    norm       row_ref's chain with e_pre in place of es;  the dropout product: one more u;  the backward's dy = dx * mask: u |dy| as
               dy_err where dropout is on;  the per-(b, i) partial rows: T_i + 1 terms
    dx0        u |acc + dx| before the output rounding
    exact      the other mix forms, gather_pad (but its bf16 rounding: cast_rne), transpose, key_pad, the dropout mask, the zero rows of d_emb
"""
import numpy as np
import torch

import gemm_ref as G
import row_ref as R
from gemm_ref import drop_mask, rnd                                    # noqa: F401  (re-exported: the GPU file draws from them)
from row_ref import check_elem, check_exact, check_mask, ln_bwd, ln_fwd  # noqa: F401

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
U24 = R.U24
NAN = float("nan")
SEED, SITE = 1234, 7


def offsets(Ts):
    off, s = [], 0
    for t in Ts:
        off.append(s)
        s += t + 1
    return off, s


def temporal_index(Ts):
    """The host's row indices of the learned temporal embedding: 0 on aggregation rows, linspace(1, T_0, T_i) as int32 on frame rows."""
    out = []
    for t in Ts:
        out += [0] + np.linspace(1, Ts[0], t).astype(np.int32).tolist()
    return np.array(out, dtype=np.int32)


def default_labels(Ts, n_labels):
    """n_labels = 2n: aggregation row of stream i = n + i, frames = i;  n_labels = n: both = i."""
    n, out = len(Ts), []
    for i, t in enumerate(Ts):
        out += [i + n if n_labels == 2 * n else i] + [i] * t
    return np.array(out, dtype=np.int32)


def _untie(u, first_col):
    """u [B, T, d] as stored: wherever a column's maximum is held by more than one frame (two random bf16 values collide easily), the
    first of them moves one unit in the last place away from zero or towards it, whichever is upwards -- random columns have NO ties,
    so that the max aggregation's placement is never a matter of 'either' (asserted in tests/test_frontend_ref_cpu.py)."""
    it = torch.int16 if u.dtype == BF else torch.int32
    for _ in range(64):
        mx = u.max(1, keepdim=True).values
        hit = u == mx
        tied = hit.sum(1, keepdim=True) > 1
        tied[:, :, :first_col] = False
        if not bool(tied.any()):
            return u
        first = hit & (hit.to(torch.int32).cumsum(1) == 1) & tied
        bits = u.contiguous().view(it)
        step = torch.where(u > 0, 1, -1).to(it)
        u = torch.where(first, (bits + step).view(u.dtype), u)
    raise AssertionError("ties remain")


# ---- operands of one front-end call ---------------------------------------------------------------------------------------------------------
class Case:
    """Operands on the CPU, dtype-rounded where the kernels take the activation type.  NaN sits in the emb_w / modal_w rows no index names.
    ties: exact ties at the column maximum as tests/test_encoder_variants_gpu._Case seeds them (two leading rows, two trailing rows,
    three rows);  int_dx: integer-valued dx;  big_mean: sample 0 of stream 0 has frame rows of mean 1000 and spread 1e-2 (in bf16 the spread
    sits in temp: 1000 + 1e-2 z is no bf16 value);  oob: one frame row with label -1, one with n_labels, one tidx = -1, one = emb_rows."""

    def __init__(self, dtype, Ts, B, d, seed=0, ties=False, emb_rows=512, n_labels=None, int_dx=False, big_mean=False, oob=False,
                 tidx=None, masks=True):
        Ts = tuple(Ts)
        self.dtype, self.Ts, self.B, self.d, self.n = dtype, Ts, B, d, len(Ts)
        n = self.n
        self.off, self.S = offsets(Ts)
        S = self.S
        us = [G.rnd((B, t, d), seed + 10 * i) for i, t in enumerate(Ts)]
        if ties:
            assert d >= 4
            for u, t in zip(us, Ts):
                if t >= 2:
                    u[:, 0, 0] = u[:, 1, 0] = 7.0
                    u[:, t - 1, 1] = u[:, t - 2, 1] = 6.0
                if t >= 3:
                    u[:, 0, 2] = u[:, 1, 2] = u[:, t - 1, 2] = 5.0
                    u[:, 1, 3] = u[:, t - 1, 3] = 4.0
        self.temp = G.rnd((S, d), seed + 101)
        if big_mean:
            z = G.rnd((Ts[0], d), seed + 102, 1e-2)
            if dtype == F32:
                us[0][0] = 1000.0 + z
            else:
                us[0][0] = 1000.0
                self.temp[1:1 + Ts[0]] = z
        self.us = [_untie(u.to(dtype), 4 if ties else 0).reshape(B * t, d).contiguous() for u, t in zip(us, Ts)]
        g = torch.Generator().manual_seed(seed + 103)
        self.masks = [(torch.rand(B, t, generator=g) < 0.4).to(torch.uint8) for t in Ts] if masks else None
        self.emb_rows = emb_rows
        self.tidx = torch.from_numpy(temporal_index(Ts) if tidx is None else np.asarray(tidx, dtype=np.int32)).clone()
        self.n_labels = (2 * n if n_labels is None else n_labels) if n > 1 else 0
        self.labels = torch.from_numpy(default_labels(Ts, self.n_labels)).clone() if n > 1 else None
        if oob:
            assert Ts[0] >= 4
            self.tidx[1], self.tidx[2] = -1, emb_rows
            if n > 1:
                self.labels[3], self.labels[4] = -1, self.n_labels
        self.emb_w = G.rnd((emb_rows, d), seed + 104)
        named = torch.zeros(emb_rows, dtype=torch.bool)
        ok = (self.tidx >= 0) & (self.tidx < emb_rows)
        named[self.tidx[ok].long()] = True
        self.emb_w[~named] = NAN
        self.emb_read = named
        self.modal_w = None
        if n > 1:
            self.modal_w = G.rnd((self.n_labels, d), seed + 105)
            seen = torch.zeros(self.n_labels, dtype=torch.bool)
            okl = (self.labels >= 0) & (self.labels < self.n_labels)
            seen[self.labels[okl].long()] = True
            self.modal_w[~seen] = NAN
        self.gamma, self.beta = R.ln_params(d, seed + 106)
        self.dx = (G.ints((B * S, d), seed + 107) if int_dx else G.rnd((B * S, d), seed + 107)).to(dtype)

    def add_rows(self, learned):
        return add_rows(self.S, self.d, temp=None if learned else self.temp, emb_w=self.emb_w if learned else None,
                        tidx=self.tidx if learned else None, modal_w=self.modal_w, labels=self.labels)


# ---- references ---------------------------------------------------------------------------------------------------------------------------------
def _take_rows(table, index):
    """(rows [S, d] in fp64 with zeros where the index is outside the table, in-range flags): rows nobody names are never touched."""
    index = index.long()
    ok = (index >= 0) & (index < table.shape[0])
    out = torch.zeros(index.numel(), table.shape[1], dtype=F64)
    out[ok] = table.to(F64)[index[ok]]
    return out, ok


def add_rows(S, d, temp=None, emb_w=None, tidx=None, modal_w=None, labels=None):
    """(add [S, d], e_add): the per-row addend and its error."""
    if temp is not None:
        tp, has_t = temp.to(F64)[:S], torch.ones(S, dtype=torch.bool)
    elif emb_w is not None:
        tp, has_t = _take_rows(emb_w, tidx)
    else:
        tp, has_t = torch.zeros(S, d, dtype=F64), torch.zeros(S, dtype=torch.bool)
    if modal_w is not None:
        md, has_m = _take_rows(modal_w, labels)
    else:
        md, has_m = torch.zeros(S, d, dtype=F64), torch.zeros(S, dtype=torch.bool)
    add = tp + md
    return add, U24 * add.abs() * (has_t & has_m)[:, None].to(F64)


def front_fwd(us, masks, add, agg, Ts, B):
    """dict(pre [B, S, d], e_pre, key_pad uint8 [B, S], arg: per stream int64 [B, d] (first maximal frame per column))."""
    add, e_add = add
    off, S = offsets(Ts)
    d = us[0].shape[1]
    pre, e = torch.zeros(B, S, d, dtype=F64), torch.zeros(B, S, d, dtype=F64)
    key = torch.zeros(B, S, dtype=torch.uint8)
    arg = []
    for i, t in enumerate(Ts):
        u = us[i].to(F64).view(B, t, d)
        o = off[i]
        mx = u.max(1).values
        arg.append((u == mx[:, None]).to(torch.int64).argmax(1))                 # first occurrence
        if agg == "avg":
            a = u.sum(1) / t
            ea = U24 * u.abs().sum(1) + U24 * a.abs()                            # T u sum |u_t| / T;  the division
        else:
            a, ea = mx, torch.zeros_like(mx)
        pre[:, o] = add[o] + a
        e[:, o] = ea + e_add[o] + U24 * pre[:, o].abs()
        pre[:, o + 1:o + 1 + t] = add[o + 1:o + 1 + t] + u
        e[:, o + 1:o + 1 + t] = e_add[o + 1:o + 1 + t] + U24 * pre[:, o + 1:o + 1 + t].abs()
        if masks is not None:
            key[:, o + 1:o + 1 + t] = (masks[i].view(B, t) != 0).to(torch.uint8)
    return dict(pre=pre, e_pre=e, key_pad=key, arg=arg)


def norm_fwd(pre, e_pre, gamma, beta, mask=None):
    """dict(x0, e_x0, mean, rstd, e_mean, e_rstd) on pre [M, d]; mask: the fp64 multipliers of the dropout BEHIND the norm."""
    f = R.ln_fwd(pre, None, gamma, beta, es=e_pre)
    x0, e = f["y"], f["e_y"]
    if mask is not None:
        x0 = x0 * mask
        e = e * mask + U24 * x0.abs()
    return dict(x0=x0, e_x0=e, mean=f["mean"], rstd=f["rstd"], e_mean=f["e_mean"], e_rstd=f["e_rstd"])


def norm_bwd(dx, pre, e_pre, gamma, mean, rstd, Ts, B, mask=None):
    """dict(dpre [B * S, d], e_dpre, ws [B * n, 2, d], e_ws): the backward per (sample, stream) block, so that the partial rows of
    param_ws count T_i + 1 terms."""
    off, S = offsets(Ts)
    n, d = len(Ts), pre.shape[1]
    dy = dx.to(F64)
    e_dy = None
    if mask is not None:
        dy = dy * mask
        e_dy = U24 * dy.abs()
    dpre, e = torch.zeros(B * S, d, dtype=F64), torch.zeros(B * S, d, dtype=F64)
    ws, e_ws = torch.zeros(B * n, 2, d, dtype=F64), torch.zeros(B * n, 2, d, dtype=F64)
    for b in range(B):
        for i, t in enumerate(Ts):
            r = slice(b * S + off[i], b * S + off[i] + t + 1)
            q = R.ln_bwd(dy[r], pre[r], None, gamma, mean[r], rstd[r], dy_err=None if e_dy is None else e_dy[r], es=e_pre[r])
            dpre[r], e[r] = q["ds"], q["e_ds"]
            ws[b * n + i, 0], ws[b * n + i, 1] = q["dgamma"], q["dbeta"]
            e_ws[b * n + i, 0], e_ws[b * n + i, 1] = q["e_dgamma"], q["e_dbeta"]
    return dict(dpre=dpre, e_dpre=e, ws=ws, e_ws=e_ws)


def _sum_by_key(g, eg, key, rows, B, S):
    """out[k] = sum over b and the s with key[s] == k of g[b, s] (keys outside [0, rows) enter nowhere); (out, e, count of s per k)."""
    d = g.shape[1]
    key = key.long()
    ok = (key >= 0) & (key < rows)
    kk = torch.where(ok, key, torch.zeros_like(key)).repeat(B)
    okk = ok.repeat(B)
    z = torch.zeros_like(g)
    t, a, ee = torch.where(okk[:, None], g, z), torch.where(okk[:, None], g.abs(), z), torch.where(okk[:, None], eg, z)
    out = torch.zeros(rows, d, dtype=F64).index_add_(0, kk, t)
    mag = torch.zeros(rows, d, dtype=F64).index_add_(0, kk, a)
    err = torch.zeros(rows, d, dtype=F64).index_add_(0, kk, ee)
    cnt = torch.zeros(rows, dtype=F64).index_add_(0, kk, okk.to(F64))
    return out, cnt[:, None] * U24 * mag + err, cnt / B


def front_bwd(dpre, Ts, B, agg, arg=None, e_dpre=None, labels=None, n_labels=0, tidx=None, emb_rows=0):
    """dict(du, e_du (lists per stream, [B * T_i, d]), d_modal, e_modal, d_emb, e_emb, emb_cnt) from dpre [B * S, d] (fp64) and its error."""
    off, S = offsets(Ts)
    d = dpre.shape[1]
    g = dpre.to(F64)
    eg = torch.zeros_like(g) if e_dpre is None else e_dpre
    g3, e3 = g.view(B, S, d), eg.view(B, S, d)
    du, e_du = [], []
    for i, t in enumerate(Ts):
        o = off[i]
        g0, e0 = g3[:, o:o + 1], e3[:, o:o + 1]
        fr, efr = g3[:, o + 1:o + 1 + t], e3[:, o + 1:o + 1 + t]
        if agg == "avg":
            v = fr + g0 / t
            e = efr + e0 / t + 2 * U24 * (g0 / t).abs() + U24 * v.abs()
        else:
            hit = (torch.arange(t)[None, :, None] == arg[i][:, None, :]).to(F64)
            v = fr + g0 * hit
            e = efr + e0 * hit + U24 * v.abs()
        du.append(v.reshape(B * t, d))
        e_du.append(e.reshape(B * t, d))
    out = dict(du=du, e_du=e_du)
    if labels is not None:
        out["d_modal"], out["e_modal"], out["modal_cnt"] = _sum_by_key(g, eg, labels, n_labels, B, S)
    if tidx is not None:
        out["d_emb"], out["e_emb"], out["emb_cnt"] = _sum_by_key(g, eg, tidx, emb_rows, B, S)
    return out


def mix_fwd(y, x0, take, B, S):
    t = take.bool().repeat(B)[:, None]
    return torch.where(t, y, x0)


def mix_bwd(dx, take, acc, B, S, init=False):
    """(dy, acc'): acc fp32 in, fp32 out (one IEEE addition per element, restated in float32); with init acc may be anything."""
    t = take.bool().repeat(B)[:, None]
    dy = torch.where(t, dx, torch.zeros_like(dx))
    g = dx.to(F32)
    if init:
        return dy, torch.where(t, torch.zeros_like(g), g)
    return dy, torch.where(t, acc, acc + g)


def mix_close(dx, acc):
    """(dx0 in fp64, e): before the output rounding."""
    v = acc.to(F64) + dx.to(F64)
    return v, U24 * v.abs()


def gather_pad(store, offs, idx, Tmax):
    """(out [B, Tmax, E] fp64, mask uint8 [B, Tmax]); rows of clips not in idx are never touched."""
    B, E = idx.numel(), store.shape[1]
    out = torch.zeros(B, Tmax, E, dtype=F64)
    mask = torch.ones(B, Tmax, dtype=torch.uint8)
    for b in range(B):
        c = int(idx[b])
        r0, ln = int(offs[c]), min(int(offs[c + 1] - offs[c]), Tmax)
        out[b, :ln] = store[r0:r0 + ln].to(F64)
        mask[b, :ln] = 0
    return out, mask


def cast_rne(bits):
    """fp32 bit patterns (any integer array) -> bf16 bit patterns (uint16), round to nearest even in integer arithmetic."""
    x = np.asarray(bits).astype(np.uint64) & np.uint64(0xFFFFFFFF)
    nan = (x & np.uint64(0x7FFFFFFF)) > np.uint64(0x7F800000)
    r = (x + np.uint64(0x7FFF) + ((x >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)
    q = (x >> np.uint64(16)) | np.uint64(0x40)
    return np.where(nan, q, r).astype(np.uint16)


def is_nan16(p):
    p = np.asarray(p).astype(np.uint32)
    return (p & 0x7FFF) > 0x7F80


def f32_bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy().astype(np.uint32)


def bf_bits(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().astype(np.uint16)


def bits_bf(p):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(p, dtype=np.uint16)).view(np.int16)).view(BF)


def bits_f32(p):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(p, dtype=np.uint32)).view(np.int32)).view(F32)


def cast_patterns():
    """Every 16-bit pattern p as the upper half of an fp32 word, with the six lower halves that decide a rounding: 393216 words."""
    hi = np.arange(65536, dtype=np.uint32) << 16
    lo = np.array([0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF], dtype=np.uint32)
    return (hi[:, None] | lo[None, :]).reshape(-1)


def transpose(src):
    return src.t().contiguous()


def to_storage(t, dtype):
    return t.to(F32).to(dtype)


# ---- checkers (those of row_ref, and the placement rule of the max aggregation) ---------------------------------------------------------------
def check_placement(what, du, dpre, Ts, B, arg, bnd_du):
    """Per column: du of the FIRST maximal frame carries the aggregation row's gradient, every other frame its own row only.  Judged
    against both candidates: a frame must lie inside its bound of the right one, and where the share exceeds twice the bound (so that
    the two cannot be confused) it must NOT lie inside the bound of the other."""
    off, S = offsets(Ts)
    d = dpre.shape[1]
    g3 = dpre.to(F64).view(B, S, d)
    wrong = 0
    for i, t in enumerate(Ts):
        o = off[i]
        g0, fr = g3[:, o:o + 1], g3[:, o + 1:o + 1 + t]
        hit = torch.arange(t)[None, :, None] == arg[i][:, None, :]
        got = du[i].detach().to(F64).cpu().view(B, t, d)
        b = bnd_du[i].view(B, t, d)
        right = torch.where(hit, fr + g0, fr)
        other = torch.where(hit, fr, fr + g0)
        clear = g0.abs().expand_as(fr) > 2 * b
        bad = ((got - right).abs() > b) | (clear & ((got - other).abs() <= b))
        wrong += int(bad.sum())
        assert int(hit.sum()) == B * d
    print(f"[front] {what}: placement of the max share, {wrong} wrong elements")
    assert wrong == 0, f"{what}: {wrong} elements carry (or miss) the aggregation row's gradient on the wrong frame"


def check_bits(what, got, ref, nan_class=False):
    """16- or 32-bit patterns, bit for bit (nan_class: a NaN pattern in the reference asks for any NaN pattern)."""
    g, r = np.asarray(got).reshape(-1), np.asarray(ref).reshape(-1)
    assert g.shape == r.shape, (g.shape, r.shape)
    bad = g != r
    if nan_class:
        if g.dtype.itemsize == 2:
            ng, nr = is_nan16(g), is_nan16(r)
        else:
            ng, nr = (g.astype(np.uint32) & 0x7FFFFFFF) > 0x7F800000, (r.astype(np.uint32) & 0x7FFFFFFF) > 0x7F800000
        bad = np.where(nr, ~ng, bad)
    n = int(bad.sum())
    print(f"[front] {what}: bit patterns, {n} of {g.size} differ")
    if n:
        w = np.nonzero(bad)[0][:8]
        raise AssertionError(f"{what}: {n} patterns differ, first at {w.tolist()}: got {[hex(int(v)) for v in g[w]]}, "
                             f"reference {[hex(int(v)) for v in r[w]]}")


# ---- the whole judgement of one front-end call: shared by the CPU file (on the emulation) and the GPU file (on the kernels) ----------------------
def _c(t):
    return None if t is None else t.detach().cpu()


def reference(case, agg, learned, norm, drop=None):
    """Everything the forward and backward of one option combination must produce: a dict of references and whole bounds.
    drop: None or (seed, site, p) of the dropout behind the norm.  The backward's statistics are the reference's, rounded to fp32."""
    c = case
    B, S, d, Ts, dt = c.B, c.S, c.d, c.Ts, c.dtype
    f = front_fwd(c.us, c.masks, c.add_rows(learned), agg, Ts, B)
    pre, e_pre = f["pre"].view(B * S, d), f["e_pre"].view(B * S, d)
    out = dict(key_pad=f["key_pad"], arg=f["arg"], pre=pre, e_pre=e_pre)
    kw = dict(labels=c.labels, n_labels=c.n_labels, tidx=c.tidx if learned else None, emb_rows=c.emb_rows)
    if not norm:
        out["x0"], out["b_x0"] = pre, R.bound(pre, e_pre, dt)
        dpre, e_dpre = c.dx.to(F64), None
    else:
        mask = G.drop_mask(B * S, d, drop) if drop is not None and drop[2] > 0 else None
        q = norm_fwd(pre, e_pre, c.gamma, c.beta, mask)
        out.update(x0=q["x0"], b_x0=R.bound(q["x0"], q["e_x0"], dt), mean=q["mean"], b_mean=R.bound(q["mean"], q["e_mean"], F32),
                   rstd=q["rstd"], b_rstd=R.bound(q["rstd"], q["e_rstd"], F32), mask=mask)
        out["mean32"], out["rstd32"] = q["mean"].to(F32), q["rstd"].to(F32)
        w = norm_bwd(c.dx, pre, e_pre, c.gamma, out["mean32"], out["rstd32"], Ts, B, mask)
        dpre, e_dpre = w["dpre"], w["e_dpre"]
        out.update(dpre=dpre, b_dpre=R.bound(dpre, e_dpre, F32), ws=w["ws"].view(-1, d), b_ws=R.bound(w["ws"], w["e_ws"], F32).view(-1, d))
    out["dpre_ref"] = dpre
    r = front_bwd(dpre, Ts, B, agg, f["arg"], e_dpre, **kw)
    out["du"], out["b_du"] = r["du"], [R.bound(v, e, dt) for v, e in zip(r["du"], r["e_du"])]
    if c.n > 1:
        out["d_modal"], out["b_modal"] = r["d_modal"], R.bound(r["d_modal"], r["e_modal"], F32)
    if learned:
        out["d_emb"], out["b_emb"], out["emb_cnt"] = r["d_emb"], R.bound(r["d_emb"], r["e_emb"], F32), r["emb_cnt"]
    return out


def judge(tag, got, ref, case, agg, norm, exact_sums=False):
    """got: dict of what the kernels (or the emulation) wrote -- any of x0, mean, rstd, key_pad, du (list), dpre, ws, d_modal, d_emb.
    Returns the worst |delta| / bound.  exact_sums: integer-valued dx without the norm -- d_modal / d_emb bit for bit."""
    w = [0.0]
    got = {k: ([_c(t) for t in v] if isinstance(v, (list, tuple)) else _c(v)) for k, v in got.items()}
    if "x0" in got:
        w.append(check_elem(f"{tag} x0", got["x0"], ref["x0"], ref["b_x0"]))
        if norm and ref.get("mask") is not None:
            check_mask(f"{tag} x0 mask", got["x0"], ref["x0"], ref["b_x0"])
    for k in ("mean", "rstd"):
        if k in got:
            w.append(check_elem(f"{tag} {k}", got[k], ref[k], ref["b_" + k]))
    if got.get("key_pad") is not None:
        check_exact(f"{tag} key_pad", got["key_pad"].view(torch.uint8), ref["key_pad"])
    if "dpre" in got:
        w.append(check_elem(f"{tag} dpre", got["dpre"], ref["dpre"], ref["b_dpre"]))
    if "ws" in got:
        w.append(check_elem(f"{tag} param_ws", got["ws"], ref["ws"], ref["b_ws"]))
    if "du" in got:
        for i, (g, r, b) in enumerate(zip(got["du"], ref["du"], ref["b_du"])):
            w.append(check_elem(f"{tag} du[{i}]", g, r, b))
        if agg == "max":
            check_placement(tag, got["du"], ref["dpre_ref"] if "dpre" not in got else got["dpre"], case.Ts, case.B, ref["arg"],
                            ref["b_du"] if "dpre" not in got else [2 * b for b in ref["b_du"]])
    if "d_modal" in got:
        if exact_sums:
            check_exact(f"{tag} d_modal", got["d_modal"], ref["d_modal"], F32)
        w.append(check_elem(f"{tag} d_modal", got["d_modal"], ref["d_modal"], ref["b_modal"]))
    if "d_emb" in got:
        read = ref["emb_cnt"] > 0
        if exact_sums:
            check_exact(f"{tag} d_emb", got["d_emb"], ref["d_emb"], F32)
        w.append(check_elem(f"{tag} d_emb (read rows)", got["d_emb"][read], ref["d_emb"][read], ref["b_emb"][read]))
        z = got["d_emb"][~read]
        nz = int((z.contiguous().view(torch.int32) != 0).sum()) if z.numel() else 0
        print(f"[front] {tag} d_emb: {int((~read).sum())} unread rows, {nz} elements that are not +0")
        assert nz == 0, f"{tag}: d_emb rows nobody reads must be +0 bit for bit"
    return max(w)


# ---- float32 emulation of each operation, with one seeded fault ----------------------------------------------------------------------------------
FAULTS = {
    "avg_divides_by_T_plus_1": "front", "avg_drops_last_frame": "front", "temporal_row_shifted": "front", "agg_row_takes_frame_label": "front",
    "max_credits_last_tie": "front", "share_not_divided": "front", "modal_drops_past_64": "front", "emb_once_per_reader": "front",
    "emb_unread_unwritten": "front", "oob_label_clamped": "front", "one_pass_variance": "front", "drop_counter_row_in_stream": "front",
    "key_pad_agg_first_mask": "front", "pad_keeps_row_0": "gather", "cast_truncates": "cast", "cast_no_exponent_carry": "cast",
    "transpose_drops_tail": "transpose", "mix_accumulates_continuing": "mix",
}


def _f(t):
    return None if t is None else t.detach().to(F32)


def _rows32(table, index, clamp=False):
    index = index.long()
    ok = (index >= 0) & (index < table.shape[0])
    out = torch.zeros(index.numel(), table.shape[1], dtype=F32)
    out[ok] = table.to(F32)[index[ok]]
    if clamp:
        out[~ok] = table.to(F32)[0]
    return out


def _drop32(case, drop, fault):
    if drop is None or drop[2] <= 0:
        return None
    B, S, d = case.B, case.S, case.d
    if fault != "drop_counter_row_in_stream":
        return G.drop_mask(B * S, d, drop).to(F32)
    m = torch.zeros(B, S, d, dtype=F32)
    for i, t in enumerate(case.Ts):
        m[:, case.off[i]:case.off[i] + t + 1] = G.drop_mask(t + 1, d, drop).to(F32)[None]
    return m.view(B * S, d)


def emulate_front(case, agg, learned, norm, drop=None, fault=None):
    """The forward and backward of one option combination in float32, as a correct kernel computes them (its summation order is one of
    those the bounds grant), with at most one fault.  Returns the dict that judge() takes."""
    assert fault is None or FAULTS[fault] == "front", fault
    c = case
    B, S, d, Ts, n, dt = c.B, c.S, c.d, c.Ts, c.n, c.dtype
    rows = torch.arange(S)
    if fault == "temporal_row_shifted":
        rows = torch.clamp(rows + 1, max=S - 1)
    tp = _rows32(c.emb_w, c.tidx[rows]) if learned else c.temp[rows]
    add = tp
    labels = None
    if n > 1:
        labels = c.labels.clone()
        if fault == "agg_row_takes_frame_label":
            for i in range(n):
                labels[c.off[i]] = labels[c.off[i] + 1]
        add = tp + _rows32(c.modal_w, labels, clamp=fault == "oob_label_clamped")
    pre = torch.zeros(B, S, d, dtype=F32)
    key = torch.zeros(B, S, dtype=torch.uint8)
    arg = []
    for i, t in enumerate(Ts):
        u = _f(c.us[i]).view(B, t, d)
        o = c.off[i]
        am = torch.zeros(B, d, dtype=torch.int64)
        val = u[:, 0].clone()
        for k in range(1, t):
            better = (u[:, k] >= val) if fault == "max_credits_last_tie" else (u[:, k] > val)
            am = torch.where(better, torch.full_like(am, k), am)
            val = torch.where(better, u[:, k], val)
        arg.append(am)
        if agg == "avg":
            acc = torch.zeros(B, d, dtype=F32)
            for k in range(t - 1 if (fault == "avg_drops_last_frame" and t > 1) else t):
                acc = acc + u[:, k]
            val = acc / float(t + 1 if fault == "avg_divides_by_T_plus_1" else t)
        pre[:, o] = add[o] + val
        pre[:, o + 1:o + 1 + t] = add[o + 1:o + 1 + t] + u
        if c.masks is not None:
            key[:, o + 1:o + 1 + t] = (c.masks[i] != 0).to(torch.uint8)
            if fault == "key_pad_agg_first_mask":
                key[:, o] = key[:, o + 1]
    pre = pre.view(B * S, d)
    out = dict(key_pad=key)
    dxf = _f(c.dx)
    if norm:
        g, bta = _f(c.gamma), _f(c.beta)
        mean = pre.sum(1) / d
        if fault == "one_pass_variance":
            var = torch.clamp((pre * pre).sum(1) / d - mean * mean, min=0.0)
        else:
            var = ((pre - mean[:, None]) ** 2).sum(1) / d
        rstd = 1.0 / torch.sqrt(var + torch.tensor(R.EPS, dtype=F32))
        y = (pre - mean[:, None]) * rstd[:, None] * g + bta
        m = _drop32(c, drop, fault)
        if m is not None:
            y = y * m
        out.update(x0=y.to(dt), mean=mean, rstd=rstd)
        # backward from the REFERENCE's statistics (the operands the GPU file hands the kernel)
        ref = R.ln_fwd(front_fwd(c.us, c.masks, c.add_rows(learned), agg, Ts, B)["pre"].view(B * S, d), None, c.gamma, c.beta)
        mean_b, rstd_b = ref["mean"].to(F32)[:, None], ref["rstd"].to(F32)[:, None]
        gy = dxf if m is None else dxf * m
        xh = (pre - mean_b) * rstd_b
        wv = gy * g
        c1, c2 = wv.sum(1, keepdim=True) / d, (wv * xh).sum(1, keepdim=True) / d
        dpre = rstd_b * (wv - c1 - xh * c2)
        ws = torch.zeros(B * n, 2, d, dtype=F32)
        for b in range(B):
            for i, t in enumerate(Ts):
                r = slice(b * S + c.off[i], b * S + c.off[i] + t + 1)
                ws[b * n + i, 0], ws[b * n + i, 1] = (gy[r] * xh[r]).sum(0), gy[r].sum(0)
        out.update(dpre=dpre, ws=ws.view(-1, d))
    else:
        out["x0"] = pre.to(dt)
        dpre = dxf
    g3 = dpre.view(B, S, d)
    du = []
    for i, t in enumerate(Ts):
        o = c.off[i]
        g0, fr = g3[:, o:o + 1], g3[:, o + 1:o + 1 + t]
        if agg == "avg":
            v = fr + (g0 if fault == "share_not_divided" else g0 / float(t))
        else:
            hit = torch.arange(t)[None, :, None] == arg[i][:, None, :]
            v = fr + torch.where(hit, g0.expand_as(fr), torch.zeros_like(fr))
        du.append(v.reshape(B * t, d).to(dt))
    out["du"] = du

    def sums(key, nrows, per_reader=False, clamp=False):
        res = torch.zeros(nrows, d, dtype=F32)
        groups = {}
        for s, k in enumerate(key.tolist()):
            if not 0 <= k < nrows:
                if not clamp:
                    continue
                k = 0
            groups.setdefault(k, []).append(s)
        for k, ss in groups.items():
            items = [(b, s) for b in range(B) for s in ss]
            if fault == "modal_drops_past_64" and not per_reader:
                items = items[:64]
            if items:
                idx = torch.tensor([b * S + s for b, s in items])
                lanes = [dpre[idx[j::64]].sum(0) for j in range(min(64, len(items)))]      # 64 lanes, a residue class each, then in lane order
                tot = torch.zeros(d, dtype=F32)
                for v in lanes:
                    tot = tot + v
                res[k] = tot * float(len(ss)) if (per_reader and fault == "emb_once_per_reader") else tot
        return res
    if n > 1:
        out["d_modal"] = sums(labels if fault == "agg_row_takes_frame_label" else c.labels, c.n_labels, clamp=fault == "oob_label_clamped")
    if learned:
        de = sums(c.tidx, c.emb_rows, per_reader=True)
        if fault == "emb_unread_unwritten":
            de[~c.emb_read] = NAN
        out["d_emb"] = de
    return out


def emulate_gather(store, offs, idx, Tmax, dtype=F32, fault=None):
    B, E = idx.numel(), store.shape[1]
    out = torch.zeros(B, Tmax, E, dtype=F32)
    mask = torch.ones(B, Tmax, dtype=torch.uint8)
    for b in range(B):
        r0, ln = int(offs[int(idx[b])]), min(int(offs[int(idx[b]) + 1] - offs[int(idx[b])]), Tmax)
        out[b, :ln] = store[r0:r0 + ln]
        mask[b, :ln] = 0
        if fault == "pad_keeps_row_0" and ln < Tmax and r0 < store.shape[0]:
            out[b, ln:] = store[r0]
    return (out if dtype == F32 else bits_bf(emulate_cast(f32_bits(out))).view(B, Tmax, E)), mask


def emulate_cast(bits, fault=None):
    """A second statement of the conversion (compare, then add): not cast_rne's formula."""
    x = np.asarray(bits).astype(np.uint32)
    hi, lo = (x >> 16).astype(np.uint32), x & 0xFFFF
    nan = (x & 0x7FFFFFFF) > 0x7F800000
    if fault == "cast_truncates":
        return np.where(nan, hi | 0x40, hi).astype(np.uint16)
    upw = (lo > 0x8000) | ((lo == 0x8000) & ((hi & 1) == 1))
    r = hi + upw.astype(np.uint32)
    if fault == "cast_no_exponent_carry":
        full = (hi & 0x7F) == 0x7F
        r = np.where(upw & full, hi & 0xFF80, r)
    return np.where(nan, hi | 0x40, r).astype(np.uint16)


def emulate_transpose(src, fault=None):
    out = src.t().contiguous().clone()
    if fault == "transpose_drops_tail":
        cols = src.shape[1]
        out[cols // 8 * 8:] = 0
    return out


def emulate_mix_bwd(dx, take, acc, B, S, init=False, fault=None):
    t = take.bool().repeat(B)[:, None]
    dy = torch.where(t, dx, torch.zeros_like(dx))
    g = dx.to(F32)
    if init:
        return dy, torch.where(t, torch.zeros_like(g), g)
    if fault == "mix_accumulates_continuing":
        return dy, acc + g
    return dy, torch.where(t, acc, acc + g)


# ---- shapes: the smallest at which each kernel can still go wrong (beside each entry: the loop trip it is there for) ------------------------------
COMBOS = tuple((agg, learned, norm) for agg in ("avg", "max") for learned in (False, True) for norm in (False, True))
SHAPES = dict(
    # enc_frontend_ex register iterations: a row lives in one wave, MAXIT vectors per lane; it >= 1 from d > 256 (fp32) / 512 (bf16); fp32
    # d = 1024 fills all four.  Each width, and one vector more.  Six rows of stream 0: the wave loop's second trip; a T = 1 stream.
    ex_regs=dict(B=2, Ts=(5, 1), d={F32: (4, 256, 260, 512, 516, 768, 772, 1020, 1024), BF: (8, 512, 520, 1016, 1024)}),
    # fx_sum_rows / the d_modal loop of mm_frontend_bwd: 64 row lanes, stride 64 over B * cnt items; every label and the embedding row
    # the four aggregation rows share have B * cnt >= 68: the second trip
    lane_wrap=dict(B=17, Ts=(5, 3, 2, 1), d=64),
    # the zeroing workgroups of d_emb: 8 workgroups, slices of 1024 flags; emb_rows < 8: workgroups that own nothing; 8200: per = 1025,
    # a second slice of one row in every workgroup (row 1024 is read, row 8199 is not)
    zero_slices=((1, (3,), (0, 0, 1, 0)), (3, (3,), (0, 1, 1, 3)), (512, (3,), None), (8200, (3, 2), (0, 1, 2, 1024, 0, 1, 3))),
    zero_d=16,
    # loops of stride 256 over frames: key_pad, fx_du_rows (Tn * nvec > 256), the frame-row loop of mm_frontend_fwd; S = 1024 is the limit
    long_one=dict(B=2, Ts=(1023,), d={F32: 4, BF: 8}),
    # the first-reader scan s < s0 of fx_sums, second trip: rows 280 .. 303 read the embedding rows 260 .. 283, whose first readers sit
    # behind row 256
    long_scan=dict(B=2, Ts=(300, 2), d=8),
    mm_long=dict(B=1, Ts=(1021, 1), d=8),
    oob=dict(B=2, Ts=(5, 2), d=8),
    drop_p=(0.1, 0.5), drop_d=(72, 520),
    big_mean_d=(8, 64),
    ties=dict(B=2, Ts=(5, 3, 2), d=8),
    # mm_frontend_fwd's aggregation-row loop: stride 256 over vectors, second trip from d > 1024 (fp32) / 2048 (bf16)
    mm_d={F32: (8, 64, 72, 1024, 1028), BF: (8, 64, 72, 1024, 2056)},
    # vct_enc_frontend_*: 128 threads, stride 128 over vectors: second trip from d > 512 (fp32) / 1024 (bf16)
    single=dict(T=(1, 3, 12), B=(1, 5), d={F32: (4, 512, 516), BF: (8, 1024, 1032)}),
    # hmm mix: one thread per vector, 256 per workgroup: totals of 1, 3 * 5 * 9 (18), 1024 * 1 (2), 2 * 7 * 128 (256) vectors -- a part
    # workgroup, whole workgroups, and both S limits
    mix={F32: ((1, 1, 4), (3, 5, 72), (1, 1024, 8), (2, 7, 1024)), BF: ((1, 1, 8), (3, 5, 72), (1, 1024, 8), (2, 7, 1024))},
    # gather: E % 4 == 0 takes the vector path (256 / 260: the 64-lane loop's second trip; 512, 1026), else the scalar path (6, 10; 1026 wraps
    # the lane loop sixteen times); B * Tmax mod 4 = 0 .. 3: the part-filled last workgroup (four rows each)
    gather_E=(4, 6, 10, 256, 260, 512, 1026), gather_BT=((4, 2), (3, 3), (2, 3), (1, 3)),
    # cast: n < 4 is the tail alone; 1023 = 255 vectors + 3; the last takes the grid-stride loop's second trip (4096 workgroups x 256
    # threads x 4 elements) and the tail
    cast_n=(1, 2, 3, 4, 5, 1023, 4 * 256 * 4096 + 7),
    # transpose: 64 x 64 tiles, vectors of 8: a tile with fewer than 8 rows, ragged columns (the scalar-load tail), more than one tile both ways
    transpose=((1, 1), (7, 9), (8, 8), (64, 64), (65, 63), (70, 130), (130, 70)),
)


def scan_tidx():
    """tidx of SHAPES['long_scan']: rows 0 .. 279 read their own embedding row, rows 280 .. 303 the rows 260 .. 283 (first read behind row
    256: found on the scan's second trip); the second stream's rows repeat rows 0 .. 2."""
    t = np.arange(304, dtype=np.int32)
    t[280:301] = t[280:301] - 20
    t[301:304] = (0, 1, 2)
    return t


def gather_case(E, B, Tmax, seed=0, zero="none"):
    """(store [rows, E] fp32, offsets int64 [n + 1], idx int64 [B]).  Clips: 0 of length Tmax, 1 of length 1, 2 (never in idx: NaN rows),
    3 of length Tmax + 2 (cut at Tmax), and with zero = "middle" a clip 4 of length 0 in front of clip 5 = NaN rows, with zero = "last" a
    clip of length 0 as the LAST clip of the store (its first row lies one past the end).  idx cycles 0, 1, 0 (a repeat), 3."""
    lens = [Tmax, 1, 2, Tmax + 2]
    if zero == "middle":
        lens += [0, 2]
    elif zero == "last":
        lens += [0]
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    store = G.rnd((int(offs[-1]), E), seed + 50)
    store[offs[2]:offs[3]] = NAN
    if zero == "middle":
        store[offs[5]:offs[6]] = NAN
    pick = [0, 1, 0, 3]
    idx = [pick[b % 4] for b in range(B)]
    if zero != "none":
        idx[B - 1] = 4
    return store, torch.from_numpy(offs), torch.tensor(idx, dtype=torch.int64)


def ex_cases(dtype, only=None):
    """Every case of vct_enc_frontend_ex_* (the CPU file runs the emulation over them, the GPU file the kernels): a list of
    (tag, Case, option combinations, dropout p or None, exact_sums).  only: the cases whose tag starts with it (the others are not built)."""
    Z = SHAPES
    learned = tuple(c for c in COMBOS if c[1])
    normed = tuple(c for c in COMBOS if c[2])
    out = []
    r = Z["ex_regs"]
    for d in r["d"][dtype]:
        out.append((f"regs d={d}", lambda d=d: Case(dtype, r["Ts"], r["B"], d, seed=d), COMBOS, None, False))
    out.append(("no masks", lambda: Case(dtype, r["Ts"], r["B"], 8, seed=3, masks=False), COMBOS, None, False))
    w = Z["lane_wrap"]
    n = len(w["Ts"])
    for nl in (2 * n, n):
        out.append((f"lane wrap n_labels={nl}", lambda nl=nl: Case(dtype, w["Ts"], w["B"], w["d"], seed=17, n_labels=nl), COMBOS, None, False))
    out.append(("lane wrap integer dx", lambda: Case(dtype, w["Ts"], w["B"], w["d"], seed=18, int_dx=True), tuple(c for c in COMBOS if not c[2]), None, True))
    for rows, Ts, tidx in Z["zero_slices"]:
        out.append((f"zero slices emb_rows={rows}", lambda rows=rows, Ts=Ts, tidx=tidx: Case(dtype, Ts, 1, Z["zero_d"], seed=rows, emb_rows=rows, tidx=tidx), learned, None, False))
    lo = Z["long_one"]
    out.append(("S=1024", lambda: Case(dtype, lo["Ts"], lo["B"], lo["d"][dtype], seed=5, emb_rows=1024), COMBOS, None, False))
    ls = Z["long_scan"]
    out.append(("first-reader scan", lambda: Case(dtype, ls["Ts"], ls["B"], ls["d"], seed=6, tidx=scan_tidx()), learned, None, False))
    o = Z["oob"]
    out.append(("out of range", lambda: Case(dtype, o["Ts"], o["B"], o["d"], seed=7, oob=True), COMBOS, None, False))
    for p in Z["drop_p"]:
        for d in Z["drop_d"]:
            out.append((f"dropout p={p} d={d}", lambda d=d: Case(dtype, r["Ts"], r["B"], d, seed=8 + d), normed, p, False))
    for d in Z["big_mean_d"]:
        out.append((f"mean 1000 d={d}", lambda d=d: Case(dtype, r["Ts"], r["B"], d, seed=9 + d, big_mean=True), normed, None, False))
    t = Z["ties"]
    out.append(("ties", lambda: Case(dtype, t["Ts"], t["B"], t["d"], seed=10, ties=True), tuple(c for c in COMBOS if c[0] == "max"), None, False))
    return [(t, c(), *rest) for t, c, *rest in out if only is None or t.startswith(only)]


def mm_cases(dtype):
    """vct_mm_frontend_*: (tag, Case, exact_sums, also accepted by enc_frontend_ex)."""
    Z = SHAPES
    r, w, m, o = Z["ex_regs"], Z["lane_wrap"], Z["mm_long"], Z["oob"]
    out = [(f"d={d}", Case(dtype, r["Ts"], r["B"], d, seed=20 + d), False, d <= 1024) for d in Z["mm_d"][dtype]]
    out.append(("lane wrap", Case(dtype, w["Ts"], w["B"], w["d"], seed=21), False, True))
    out.append(("lane wrap integer dx", Case(dtype, w["Ts"], w["B"], w["d"], seed=22, int_dx=True), True, True))
    out.append(("S=1024", Case(dtype, m["Ts"], m["B"], m["d"], seed=23), False, True))
    out.append(("out of range", Case(dtype, o["Ts"], o["B"], o["d"], seed=24, oob=True), False, True))
    out.append(("no masks", Case(dtype, r["Ts"], r["B"], 8, seed=25, masks=False), False, True))
    return out


def single_cases(dtype):
    Z = SHAPES["single"]
    return [(f"T={T} B={B} d={d}", Case(dtype, (T,), B, d, seed=30 + T + B + d, masks=False)) for T in Z["T"] for B in Z["B"] for d in Z["d"][dtype]]


def drop_of(p):
    return None if p is None else (SEED, SITE, p)
