"""fp64 references, per-element bounds, checkers, shapes and a fault-injecting float32 emulation of the memory-bound row kernels:
residual + LayerNorm forward / backward and its two-norm forms (csrc/vct_norm.hip), the dgamma / dbeta finalize, the symmetric
cross-entropy loss (vct_sce_loss, csrc/vct_caption_loss.hip), the token embedding forward / backward (csrc/vct_elem.hip) and the flat Adam step
(csrc/vct_optim.hip, vct_adam_core.h).  Shared by tests/test_row_ref_cpu.py (which checks THIS file against torch.nn.functional,
autograd, torch.optim and oracle/vct_oracle.py, and shows that every checker rejects the seeded faults) and
tests/test_row_kernels_gpu.py.  Plain torch in float64 on whatever device the operands live on; nothing here reads the library.

Operations (include/vct_hip.h and oracle/vct_oracle.py; written from the formulas, not from the kernels' code paths)
    ln_fwd    s = res + x * mask;  mean = sum s / d;  var = sum (s - mean)^2 / d (biased);  rstd = 1 / sqrt(var + 1e-5);
              y = (s - mean) rstd gamma + beta
    ln_bwd    h = (s - mean) rstd (mean, rstd: the SAVED fp32 statistics, operands of the backward);  dh = dy gamma;
              ds = rstd (dh - mean_d(dh) - h mean_d(dh h));  dxo = ds * mask;  dgamma = sum_rows dy h;  dbeta = sum_rows dy
    two norms y2 = LN2(y as STORED): the second norm is judged against ln_fwd of the y the kernel wrote (which is judged on its
              own); backwards, dy = ln_bwd of the front norm rounded to the storage type, whose bound enters the second ln_bwd as dy_err
    sce       p = softmax(x);  CE_n = lse - x_y on non-pad rows / nvalid;  RCE_n = c (Q_n + 1e-7 cnt_n), c = -log(1e-4) in fp32,
              Q = sum_{j != y, p_j >= 1e-7} p_j, cnt = #{j != y, p_j < 1e-7};  loss = alpha CE + (1 - alpha) mean_n RCE (alpha = 1: CE);
              gradient p_j (a + bn (c [p_j >= 1e-7] - c Q)) off the label, a (p_y - 1) - bn p_y c Q on it, a = alpha / nvalid on
              non-pad rows, bn = (1 - alpha) / N
    embed     x[n] = (table[id_n] + pos[n % S]) * mask;  dtable[id] = sum over the non-pad positions n of id of dx[n] * mask
    adam      torch.optim.Adam, single tensor: t = step + 1;  m += (1 - b1)(g - m);  v = b2 v + (1 - b2) g^2;
              p = p (1 - lr wd) - (lr / (1 - b1^t)) m / (sqrt(v) / sqrt(1 - b2^t) + eps);  shadow = bf16(p).  The hyper-parameters
              are the fp32 values the kernel receives (0.9 is not 0.9f: 1 - b2 would otherwise differ by 3e-5).

Bounds.  Every bound is  u_out |ref| + e,  u_out = 2^-24 (fp32 result) or 2^-8 (bf16 result), u = 2^-24, and e the first-order
propagation of one relative u per fp32 operation on the path (a rounding of a quantity z costs u |z|; an error ez of an operand of a
product z w costs ez |w|; a sum of n terms in ANY order costs n u sum |terms| plus the terms' own errors).  None is sized from the
kernels' output.
    ln_fwd    es = 2 u (|x mask| + |res|) for s (one product, one sum);  e_mean = u sum|s| + mean_d(es) + u |mean| (d terms, the
              division);  ec = es + e_mean + u |c| for c = s - mean;  e_var = mean_d(2 |c| ec + u c^2) + u sum c^2 + u var;
              rstd: the kernel's variance is >= 0, so its relative error is at most sqrt((var + eps) / max(var + eps - e_var, eps)) - 1,
              plus 4.5 u (the sum with eps, sqrtf and the division at one ulp each);  y: h = c rstd, h gamma, + beta: one u each.
              (A row of mean 1000 and spread 1e-2 has e_mean = d 6e-5: its bound is tight at small d only -- that is where the
              one-pass variance is rejected.)
    ln_bwd    the same chain for h from the saved statistics (no error of their own: they are inputs), dh, the two row means
              (d terms each), the three operations of ds, one more product for dxo;  dgamma / dbeta: M terms.
    sce       __expf / __logf carry no documented bound: SCE_EXP_REL is MEASURED on the device (test_row_kernels_gpu.py,
              test_sce_measure_exp) as max |p_kernel - p| / p over the test's own fp32 rows at alpha = 1, where the gradient is
              (p - onehot) / nvalid, and SCE_EXP_ALLOW = 4 x that figure is the relative error granted to every p, to sum exp and to
              log (other inputs reach other arguments: the factor).  The sum Q adds exact zeros for the small columns, so it counts
              nbig + 2 terms.  That MEASURED allowance (the E terms) never exceeds SCE_CAP (2e-5 fp32, 6e-3 bf16: the figures of
              tests/test_kernels_gpu.py::test_sce_loss) times the row's largest |ref|, the loss's never 2e-5 |loss|.  The cap is on
              the intrinsic term alone: u_out |ref| and the derived rounding terms are added outside it, because they cannot be
              capped by the row's largest |ref| -- in a row whose label column holds p_y = 1 - 1e-12 every reference gradient is about
              1e-12, fp32 has p_y = 1 exactly and a CORRECT kernel writes 0 in the label column (the term 3 u a (1 + p_y)).
              Beside the clamp (|p / 1e-7 - 1| <= 2^-10 in fp64) the fp32 p may fall on either side: either branch's value is
              accepted there, and sce_case() keeps the share of such elements below 1 % (asserted in the CPU file).
    embed     fwd: two roundings;  bwd: k occurrences = k products and k additions: (k + 1) u sum |dx mask|.  Integer dx at p = 0: exact.
    adam      every rounding of adam_update is a pinned intrinsic: m = fma((1 - b1), (g - m), m): 3 u (c |g - m| + |m'|);  v: four
              roundings of non-negative terms: 4 u v' (+ 4 * 2^-126: a flushed denormal);  sqrt(v), / bc2s, + eps: one u each, the
              error of v through sqrt exactly (sqrt(v + ev) - sqrt(v));  m / denom, the fma with step_size, p decay: one u each.  The
              constants: powf is granted ADAM_POW_ULPS = 2 ulp (the figure HIP's math tables give is 1; no table ships with the
              toolchain, so this is an assumption with a factor of two) -- 1 - b^t turns that into 2^-23 * ULPS * b^t / (1 - b^t).
"""
import math

import numpy as np
import torch

import gemm_ref as G

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
U24, U8 = 2.0 ** -24, 2.0 ** -8
EPS = 1e-5
SCE_C = float(np.float32(9.210340371976184))            # -log(1e-4) as the fp32 constant of kernel and oracle
CLAMP = 1e-7
NEAR = 2.0 ** -10
# measured on an MI355X by tests/test_row_kernels_gpu.py::test_sce_measure_exp: max |p_kernel - p| / p = 3.831e-6 over the fp32 rows of
# SHAPES (the far columns of the dominant rows, x - max near -45: the argument's own rounding is 45 * 2^-24 = 2.7e-6 there); factor 4
SCE_EXP_REL = 3.831e-6
SCE_EXP_ALLOW = 4.0 * SCE_EXP_REL
SCE_CAP = {F32: 2e-5, BF: 6e-3}
SCE_LOSS_CAP = 2e-5
ADAM_POW_ULPS = 2.0


def u_of(dtype):
    return U8 if dtype == BF else U24


def vec_of(dtype):
    return 8 if dtype == BF else 4


def up(x, q):
    return (x + q - 1) // q * q


def bound(ref, e, dtype):
    return u_of(dtype) * ref.abs() + e


def drop_mask(rows, cols, drop, device="cpu"):
    """fp64 multipliers [rows, cols] of dropout (seed, site, p): counter = row * cols + col (layer_ss_ref.drop_mult)."""
    return G.drop_mask(rows, cols, drop, device)


def rnd(shape, seed, scale=1.0, dtype=F32, device="cpu"):
    return G.rnd(shape, seed, scale, dtype, device)


# ---- LayerNorm ------------------------------------------------------------------------------------------------------------------------------
def _presum(x, res, mask):
    x = x.to(F64)
    xm = x if mask is None else x * mask.to(x.device)
    if res is None:
        return xm, xm.abs(), U24 * xm.abs() * (0.0 if mask is None else 1.0)
    r = res.to(F64)
    return xm + r, xm.abs() + r.abs(), 2 * U24 * (xm.abs() + r.abs())


def ln_fwd(x, res, gamma, beta, mask=None, es=None):
    """dict(y, mean, rstd, e_y, e_mean, e_rstd): references and the error terms e of the module docstring (u_out |ref| not included).
    es: the error of the norm's input s where it is not the one product and one sum of _presum (tests/frontend_ref.py)."""
    s, _, es0 = _presum(x, res, mask)
    es = es0 if es is None else es.to(s.device)
    g, b = gamma.to(F64).to(s.device), beta.to(F64).to(s.device)
    d = s.shape[1]
    mean = s.mean(1)
    c = s - mean[:, None]
    var = (c * c).mean(1)
    rstd = 1.0 / torch.sqrt(var + EPS)
    y = c * rstd[:, None] * g + b
    e_mean = U24 * s.abs().sum(1) + es.sum(1) / d + U24 * mean.abs()
    ec = es + e_mean[:, None] + U24 * c.abs()
    e_var = (2 * c.abs() * ec + U24 * c * c).sum(1) / d + U24 * (c * c).sum(1) + U24 * var
    e_r = torch.sqrt((var + EPS) / torch.clamp(var + EPS - e_var, min=EPS)) - 1.0 + 4.5 * U24      # relative
    h = c * rstd[:, None]
    eh = ec * rstd[:, None] + h.abs() * (e_r[:, None] + U24)
    e_y = eh * g.abs() + U24 * (h * g).abs() + U24 * y.abs()
    return dict(y=y, mean=mean, rstd=rstd, e_y=e_y, e_mean=e_mean, e_rstd=rstd * e_r)


def ln_bwd(dy, x, res, gamma, mean, rstd, mask=None, dy_err=None, es=None):
    """dict(ds, dxo, dgamma, dbeta, e_ds, e_dxo, e_dgamma, e_dbeta).  mean / rstd: the saved statistics (exact operands); es as in ln_fwd."""
    s, _, es0 = _presum(x, res, mask)
    es = es0 if es is None else es.to(s.device)
    dev = s.device
    M, d = s.shape
    g, dy = gamma.to(F64).to(dev), dy.to(F64).to(dev)
    mean, rstd = mean.to(F64).to(dev)[:, None], rstd.to(F64).to(dev)[:, None]
    m = torch.ones_like(s) if mask is None else mask.to(dev)
    e_dy = torch.zeros_like(s) if dy_err is None else dy_err.to(dev)
    cm = s - mean
    h = cm * rstd
    eh = (es + U24 * cm.abs()) * rstd + U24 * h.abs()
    dh = dy * g
    edh = U24 * dh.abs() + e_dy * g.abs()
    c1 = dh.mean(1, keepdim=True)
    e_c1 = U24 * dh.abs().sum(1, keepdim=True) + edh.sum(1, keepdim=True) / d + U24 * c1.abs()
    t = dh * h
    et = dh.abs() * eh + h.abs() * edh + U24 * t.abs()
    c2 = t.mean(1, keepdim=True)
    e_c2 = U24 * t.abs().sum(1, keepdim=True) + et.sum(1, keepdim=True) / d + U24 * c2.abs()
    a, b = dh - c1, h * c2
    ea = edh + e_c1 + U24 * a.abs()
    eb = eh * c2.abs() + h.abs() * e_c2 + U24 * b.abs()
    w = a - b
    v = rstd * w
    ev = rstd * (ea + eb + U24 * w.abs()) + U24 * v.abs()
    tg = dy * h
    etg = dy.abs() * eh + e_dy * h.abs() + U24 * tg.abs()
    return dict(ds=v, dxo=v * m, dgamma=tg.sum(0), dbeta=dy.sum(0), e_ds=ev, e_dxo=(ev + U24 * v.abs()) * m,
                e_dgamma=M * U24 * tg.abs().sum(0) + etg.sum(0), e_dbeta=M * U24 * dy.abs().sum(0) + e_dy.sum(0))


def to_storage(t, dtype):
    """fp64 -> the storage type (round to nearest even), back in fp64."""
    return t.to(F32).to(dtype).to(F64)


def ln_rows(M, d, seed, dtype, with_res, device="cpu"):
    """(x, res) [M, d] of `dtype`: row r is random, of mean 1000 and spread 1e-2, constant, zero, random for r % 5 = 0 .. 4 (in bf16 the
    spread of the second kind sits in res: 1000 + 1e-2 z is not a bf16 value)."""
    x = G.rnd((M, d), seed, 1.0, F32)
    r = G.rnd((M, d), seed + 1, 1.0, F32)
    z = G.rnd((M, d), seed + 2, 1e-2, F32)
    for i in range(M):
        k = i % 5
        if k == 1:
            x[i], r[i] = (1000.0 + z[i], 0.0) if dtype == F32 else (1000.0, z[i])
        elif k == 2:
            x[i], r[i] = 1.5, 0.25
        elif k == 3:
            x[i], r[i] = 0.0, 0.0
    return x.to(dtype).to(device), (r.to(dtype).to(device) if with_res else None)


def ln_params(d, seed, device="cpu"):
    return (1.0 + 0.1 * G.rnd((d,), seed)).to(device), (0.1 * G.rnd((d,), seed + 1)).to(device)


# ---- symmetric cross-entropy ---------------------------------------------------------------------------------------------------------------
def sce(logits, labels, alpha, pad_id, dtype=F32, e_exp=None):
    """logits [N, V] (valid columns only), labels [N] int64.  dict(loss, grad, alt, near, ce_rows, rce_rows, p, b_grad, b_ce, b_rce, b_loss: the whole bounds): alt = the value of
    the other branch of the p >= 1e-7 test (equal to grad away from the clamp), near = the elements beside it.  A label outside
    [0, V) is computed against column 0 and makes a NaN loss when the row counts (the kernel's documented guard)."""
    E = SCE_EXP_ALLOW if e_exp is None else e_exp
    x = logits.to(F64)
    N, V = x.shape
    lab = labels.to(x.device).reshape(-1)
    rows = torch.arange(N, device=x.device)
    valid = lab != pad_id
    oob = (lab < 0) | (lab >= V)
    y = torch.where(oob, torch.zeros_like(lab), lab)
    nvalid = float(valid.sum())
    mx = x.max(1).values
    e = torch.exp(x - mx[:, None])
    se = e.sum(1)
    p = e / se[:, None]
    lse = mx + torch.log(se)
    xy, py = x[rows, y], p[rows, y]
    ce_rows = torch.where(valid, lse - xy, torch.zeros_like(lse))
    ce_rows = torch.where(valid & oob, torch.full_like(lse, float("nan")), ce_rows)
    off = torch.ones_like(p, dtype=torch.bool)
    off[rows, y] = False
    big = p >= CLAMP
    one = alpha == 1.0
    beta = 0.0 if one else 1.0 - alpha
    near = ((p / CLAMP - 1.0).abs() <= NEAR) & off & (not one)
    Q = (p * (big & off)).sum(1)
    cnt = ((~big) & off).sum(1).to(F64)
    nbig = (big & off).sum(1).to(F64)
    rce_rows = SCE_C * (Q + CLAMP * cnt)
    a = valid.to(F64) * (alpha / nvalid if nvalid else float("nan"))
    bn = beta / N
    k_small = (a - bn * SCE_C * Q)[:, None]
    k_big = k_small + bn * SCE_C
    grad = p * torch.where(big, k_big, k_small)
    alt = p * torch.where(big, k_small, k_big)
    gy = a * (py - 1.0) - bn * py * SCE_C * Q
    grad[rows, y] = gy
    alt[rows, y] = gy
    alt = torch.where(near, alt, grad)                  # the other branch is acceptable BESIDE the clamp only
    loss = ce_rows.sum() / nvalid if nvalid else torch.tensor(float("nan"), dtype=F64, device=x.device)
    if not one:
        loss = alpha * loss + beta * rce_rows.mean()
    # bounds: the rounding terms (u) and the __expf / __logf terms (E) apart -- the cap applies to the second kind only
    near_p = (p * near).sum(1)
    Qa = Q + torch.where(big[rows, y], py, torch.zeros_like(py))          # what the kernel sums before it takes the label column out
    eQ_u, eQ_E = Qa * (nbig + 2) * U24 + near_p, Qa * 2 * E
    eK_u = (2 * U24 * a.abs() + bn * SCE_C * eQ_u + 3 * U24 * (a.abs() + bn * SCE_C * (Q + 1.0)))[:, None]
    eK_E = (bn * SCE_C * eQ_E)[:, None]
    eg_u = p * eK_u + grad.abs() * 2 * U24
    eg_E = p * eK_E + grad.abs() * E
    eg_u[rows, y] = a.abs() * 3 * U24 * (1.0 + py) + bn * SCE_C * py * (eQ_u + Q * 3 * U24)
    eg_E[rows, y] = a.abs() * py * E + bn * SCE_C * py * (eQ_E + Q * E)
    rowmax = grad.abs().max(1, keepdim=True).values
    capped = bound(grad, eg_u, dtype) + torch.minimum(eg_E, SCE_CAP[dtype] * rowmax.expand_as(eg_E))
    lg = torch.log(se).abs()
    zero = torch.zeros_like(lse)
    ece_u = torch.where(valid, 3 * U24 * (mx.abs() + lg + xy.abs()) + U24 * ce_rows.abs(), zero)
    ece_E = torch.where(valid, E * (1.0 + lg), zero)
    erce_u = SCE_C * (eQ_u + CLAMP * (near.sum(1).to(F64) + 2 * U24 * cnt)) + 2 * U24 * rce_rows
    erce_E = SCE_C * eQ_E
    nv = max(nvalid, 1.0)
    el_u, el_E = (ece_u.sum() + N * U24 * ce_rows.abs().sum()) / nv, ece_E.sum() / nv
    if not one:
        el_u = alpha * el_u + beta * (erce_u.sum() + N * U24 * rce_rows.sum()) / N
        el_E = alpha * el_E + beta * erce_E.sum() / N
    e_loss = el_u + 4 * U24 * loss.abs() + torch.minimum(el_E, SCE_LOSS_CAP * loss.abs())
    e_ce, e_rce = ece_u + ece_E, erce_u + erce_E
    return dict(loss=loss, grad=grad, alt=alt, near=near, ce_rows=ce_rows, rce_rows=rce_rows, p=p, valid=valid, nvalid=nvalid, y=y,
                b_grad=capped, b_ce=bound(ce_rows, e_ce, F32), b_rce=bound(rce_rows, e_rce, F32), b_loss=e_loss, small=((~big) & off),
                py=py)


def sce_pad_id(V):
    return 1 if V >= 4 else -1


def sce_case(V, seed, dtype, B=3, S=2, oob=False):
    """(logits [N, V] of dtype on the CPU, ids [B, S + 1] int64, pad_id): N = B * S rows seen through the shifted-label view ids[:, 1:].
    Row 0: label in column 0, which dominates (every other p < 1e-7, Q = 0);  row 1: label in column V - 1 with column 0 dominant
    (the label column is below the clamp);  row 2: a random row, label in the middle;  row 3: the pad tail of its sequence;  rows 4, 5:
    an all-pad sequence.  Random logits 3 z; a dominant column holds 32, at least 18 above every other (z < 4.6 at V = 65536)."""
    N = B * S
    x = G.rnd((N, V), seed, 3.0, F32)
    x[0, 0] = 32.0
    if V > 1:
        x[1, 0] = 32.0
    pad = sce_pad_id(V)
    mid = min(max(V // 2, 2), V - 1) if V >= 4 else V // 2
    lab = torch.full((N,), pad, dtype=torch.int64)
    lab[0], lab[1], lab[2] = 0, V - 1, mid
    if oob:
        lab[2] = V
    ids = torch.full((B, S + 1), pad, dtype=torch.int64)
    ids[:, 1:] = lab.view(B, S)
    ids[:, 0] = 0
    return x.to(dtype), ids, pad


def sce_tile(V, ld_dl, dtype):
    """Register-tile columns IT * NT * VEC of the instantiation vct_sce_loss picks (ld_dl = 0: forward only), and its name."""
    vec = vec_of(dtype)
    width = max(up(V, vec), ld_dl)
    small = width <= 4096 * vec
    name = {(BF, True): "bf16 512x8", (BF, False): "bf16 1024x8", (F32, True): "fp32 1024x4", (F32, False): "fp32 1024x8"}[(dtype, small)]
    return (4096 if small else 8192) * vec, name


# ---- embedding -------------------------------------------------------------------------------------------------------------------------------
def embed_fwd(ids, table, pos, S, mask=None):
    """ids [N] (all inside the table), table [V, d], pos [>= S, d]: (x [N, d], e)."""
    N = ids.numel()
    t = table.to(F64)[ids.reshape(-1)] + pos.to(F64)[torch.arange(N, device=ids.device) % S]
    x = t if mask is None else t * mask.to(t.device)
    return x, U24 * t.abs() * (x != 0) + U24 * x.abs()


def embed_bwd(ids, dx, V, pad_id, mask=None):
    """(dtable [V, d], e, count [V]): positions whose id is pad_id or outside [0, V) own no row."""
    idf = ids.reshape(-1)
    ok = (idf != pad_id) & (idf >= 0) & (idf < V)
    t = dx.to(F64) if mask is None else dx.to(F64) * mask.to(dx.device)
    t = torch.where(ok[:, None], t, torch.zeros_like(t))                   # (NaN in the rows nobody may read never enters)
    idc = torch.where(ok, idf, torch.zeros_like(idf))
    out = torch.zeros(V, t.shape[1], dtype=F64, device=t.device).index_add_(0, idc, t)
    mag = torch.zeros_like(out).index_add_(0, idc, t.abs())
    cnt = torch.zeros(V, dtype=F64, device=t.device).index_add_(0, idc, ok.to(F64))
    return out, (cnt[:, None] + 1) * U24 * mag, cnt


def embed_ids(kind, V=None):
    """ids [B, S + 1] int64 (the first S columns are used: the batch-stride view), S, V, pad_id = 0.
    "mixed": 300 positions -- token 5 forty times, 6 nine times, 7 eight times, 8 once, pads, one id equal to V, one -1, the rest
    distinct tokens (once each), in a fixed shuffle;  "same": 1100 positions of token 3;  "far": 1100 positions of token 3 but eight of
    token 4, the first at position 1 and the last at 1098 (a light token whose scan takes a second 1024-position trip)."""
    if kind == "mixed":
        B, S, V = 30, 10, 320
        flat = [5] * 40 + [6] * 9 + [7] * 8 + [8] + [0] * 12 + [V, -1]
        flat += list(range(10, 10 + B * S - len(flat)))
        perm = np.random.RandomState(7).permutation(B * S)
        flat = torch.tensor(flat, dtype=torch.int64)[torch.from_numpy(perm)]
    else:
        B, S, V = 110, 10, 8
        flat = torch.full((B * S,), 3, dtype=torch.int64)
        if kind == "far":
            flat[[1, 200, 400, 600, 800, 1000, 1050, 1098]] = 4
    ids = torch.full((B, S + 1), 2, dtype=torch.int64)
    ids[:, :S] = flat.view(B, S)
    return ids, S, V, 0


# ---- Adam -----------------------------------------------------------------------------------------------------------------------------------
def f32v(x):
    return float(np.float32(x))


def adam(p, g, m, v, lr, b1, b2, eps, wd, step):
    """One step, t = step + 1.  dict(p, m, v, e_p, e_m, e_v); hyper-parameters as the fp32 values the kernel is given."""
    lr, b1, b2, eps, wd = (f32v(z) for z in (lr, b1, b2, eps, wd))
    p, g, m, v = (z.to(F64) for z in (p, g, m, v))
    t = step + 1
    pw1, pw2 = b1 ** t, b2 ** t
    bc1, bc2 = 1.0 - pw1, 1.0 - pw2
    c1 = 1.0 - b1
    m2 = m + c1 * (g - m)
    v2 = b2 * v + (1.0 - b2) * g * g
    decay = 1.0 - lr * wd
    w0 = p * decay
    sq = torch.sqrt(v2)
    denom = sq / math.sqrt(bc2) + eps
    ss = lr / bc1
    q = m2 / denom
    p2 = w0 - ss * q
    # bounds
    e_m = 3 * U24 * (c1 * (g - m).abs() + m2.abs())
    e_v = 4 * U24 * v2 + 4 * 2.0 ** -126
    e_bc1 = ADAM_POW_ULPS * 2.0 ** -23 * pw1 / bc1 + U24
    e_bc2s = 0.5 * (ADAM_POW_ULPS * 2.0 ** -23 * pw2 / bc2 + U24) + U24
    e_sq = torch.sqrt(v2 + e_v) - sq + U24 * sq
    sb = sq / math.sqrt(bc2)
    e_den = e_sq / math.sqrt(bc2) + sb * (e_bc2s + U24) + U24 * denom
    e_q = e_m / denom + q.abs() * (e_den / denom + U24)
    e_p = 3 * U24 * w0.abs() + ss * (e_q + q.abs() * (e_bc1 + 2 * U24)) + U24 * p2.abs()
    return dict(p=p2, m=m2, v=v2, e_p=1.01 * e_p, e_m=e_m, e_v=e_v)          # 1.01: the second-order terms of a first-order bound


def adam_case(n, seed, device="cpu"):
    """(p, g, m, v) fp32 [n]: random, with the special elements of the first float4: g = m = v = 0; v = 0 with g != 0; g = 1e-20."""
    p, g = G.rnd((n,), seed, 0.5), G.rnd((n,), seed + 1, 1e-2)
    m, v = G.rnd((n,), seed + 2, 1e-2), G.rnd((n,), seed + 3, 1e-2) ** 2
    g[0] = m[0] = v[0] = 0.0
    v[1] = 0.0
    g[2], m[2], v[2] = 1e-20, 0.0, 0.0
    return p.to(device), g.to(device), m.to(device), v.to(device)


# ---- checkers -------------------------------------------------------------------------------------------------------------------------------
def _2d(t):
    return t.reshape(-1, 1) if t.dim() < 2 else t.reshape(-1, t.shape[-1])


def _like(t, g):
    """t (reference, bound) on g's device in g's shape: the element counts must agree (no broadcasting of a [n] against a [1, n])."""
    assert t.numel() == g.numel(), (tuple(t.shape), tuple(g.shape))
    return t.to(g.device).reshape(g.shape)


def check_elem(what, got, ref, bnd, alt=None):
    """|got - ref| <= bnd at every element (alt: or |got - alt| <= bnd); prints and returns the worst |delta| / bound."""
    g = _2d(got.detach().to(F64))
    r, b = _like(ref.to(F64), g), _like(bnd.to(F64), g)
    delta = (g - r).abs()
    if alt is not None:
        delta = torch.minimum(delta, (g - _like(alt.to(F64), g)).abs())
    excess = torch.nan_to_num(delta - b, nan=float("inf"))
    ratio = torch.where(delta == 0, torch.zeros_like(delta), delta / b.clamp(min=1e-300)).nan_to_num(nan=float("inf"))
    w = int(excess.argmax())
    r0, c0 = w // g.shape[1], w % g.shape[1]
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print(f"[row] {what}: worst |delta| / bound = {worst:.3f} (worst |delta| - bound = {float(excess.max()):.3e} at row {r0} column {c0})")
    assert float(excess.max()) <= 0.0, (f"{what}: row {r0} column {c0}: got {float(g[r0, c0])!r}, reference {float(r[r0, c0])!r}, "
                                        f"bound {float(b[r0, c0]):.3e}")
    return worst


def check_exact(what, got, ref, dtype=None):
    """Bit for bit: ref rounded to the output type must equal got (NaN nowhere)."""
    dtype = got.dtype if dtype is None else dtype
    g = _2d(got.detach())
    r = _like(ref.to(F32).to(dtype) if ref.dtype == F64 else ref, g)
    bad = ~(g == r)
    n = int(bad.sum())
    print(f"[row] {what}: exact, {n} of {g.numel()} elements differ")
    assert n == 0, f"{what}: {n} elements differ, first at (row, column) {bad.nonzero()[0].tolist()}: got {g[bad][0].item()!r}, reference {r[bad][0].item()!r}"


def check_mask(what, got, ref, bnd=None):
    """The elements zero in one tensor and not in the other must number 0 (gemm_ref.check_mask's rule).  ref carries the mask of
    layer_ss_ref.drop_mult (it is never read off the kernel's output); bnd: kept elements whose reference lies inside its own bound
    may round to zero and are left out (counted and printed)."""
    g = got.detach().to(F64)
    r = _like(ref.to(F64), g)
    a, b = g == 0, r == 0
    bad = a != b
    if bnd is not None:
        amb = (~b) & (r.abs() <= _like(bnd, g))
        print(f"[row] {what}: {int(amb.sum())} kept elements inside their own bound")
        bad = bad & ~amb
    n = int(bad.sum())
    print(f"[row] {what}: {int(b.sum())} zeros in the reference, {n} mismatches")
    assert n == 0, f"{what}: {n} elements zero in one and not in the other, first at {bad.nonzero()[0].tolist()}"


# ---- float32 emulation of each operation, with one seeded fault -----------------------------------------------------------------------------
FAULTS = {
    "mean_drops_last_vector": "ln_fwd", "one_pass_variance": "ln_fwd", "rstd_without_eps": "ln_fwd", "neighbour_row_statistic": "ln_fwd",
    "truncate_bf16": "ln_fwd",
    "dgamma_misses_last_partial": "ln_bwd", "dgamma_dbeta_swapped": "ln_bwd", "dxo_not_masked": "ln_bwd",
    "padding_counted_small": "sce", "label_left_in_q": "sce", "nvalid_counts_pads": "sce", "gradient_small_branch_everywhere": "sce",
    "t_is_step": "adam", "decay_after_step": "adam",
    "drop_one_occurrence": "embed_bwd",
}


def _store(x, dtype, fault=None):
    if fault == "truncate_bf16" and dtype == BF:
        return (x.contiguous().view(torch.int32) & -65536).view(F32).to(BF)
    return x.to(dtype)


def _f(t):
    return None if t is None else t.detach().to("cpu").to(F32)


def F32v(x):
    return torch.tensor(x, dtype=F32)


def emulate(op, *args, fault=None, **kw):
    """The operation `op` in float32 on the CPU, as a correct kernel computes it (any summation order is inside the bounds), with at
    most one fault of FAULTS."""
    assert fault is None or FAULTS[fault] == op, (op, fault)
    return _EMU[op](*args, fault=fault, **kw)


def _emu_ln_fwd(x, res, gamma, beta, mask=None, dtype=F32, fault=None):
    x, res, g, b = _f(x), _f(res), _f(gamma), _f(beta)
    s = x if mask is None else x * mask.to(F32)
    s = s if res is None else s + res
    d = s.shape[1]
    mean = (s[:, :d - vec_of(dtype)] if fault == "mean_drops_last_vector" else s).sum(1) / d
    if fault == "one_pass_variance":
        var = torch.clamp((s * s).sum(1) / d - mean * mean, min=0.0)
    else:
        var = ((s - mean[:, None]) ** 2).sum(1) / d
    rstd = 1.0 / torch.sqrt(var if fault == "rstd_without_eps" else var + F32v(EPS))
    if fault == "neighbour_row_statistic":
        mean = torch.roll(mean, 1)
    y = (s - mean[:, None]) * rstd[:, None] * g + b
    return _store(y, dtype, fault), mean, rstd


def _emu_ln_bwd(dy, x, res, gamma, mean, rstd, mask=None, dtype=F32, fault=None):
    dy, x, res, g, mean, rstd = _f(dy), _f(x), _f(res), _f(gamma), _f(mean)[:, None], _f(rstd)[:, None]
    m = torch.ones_like(x) if mask is None else mask.to(F32)
    s = x * m if res is None else x * m + res
    M, d = s.shape
    h = (s - mean) * rstd
    dh = dy * g
    c1, c2 = dh.sum(1, keepdim=True) / d, (dh * h).sum(1, keepdim=True) / d
    v = rstd * ((dh - c1) - h * c2)
    nws = (M + 3) // 4                                           # one partial row per four-row workgroup, summed afterwards
    pad = nws * 4 - M
    z = torch.zeros(pad, d)
    pg = torch.cat([dy * h, z]).view(nws, 4, d).sum(1)
    pb = torch.cat([dy, z]).view(nws, 4, d).sum(1)
    dg = (pg[:-1] if fault == "dgamma_misses_last_partial" else pg).sum(0)
    db = pb.sum(0)
    if fault == "dgamma_dbeta_swapped":
        dg, db = db, dg
    return _store(v, dtype), _store(v if fault == "dxo_not_masked" else v * m, dtype), dg, db


def _emu_sce(logits, labels, alpha, pad_id, dtype=F32, tile=None, fault=None):
    x = _f(logits)
    N, V = x.shape
    lab = labels.reshape(-1)
    tile = sce_tile(V, up(V, vec_of(dtype)), dtype)[0] if tile is None else tile
    rows = torch.arange(N)
    valid = lab != pad_id
    y = torch.where((lab < 0) | (lab >= V), torch.zeros_like(lab), lab)
    nvalid = F32v(float(N if fault == "nvalid_counts_pads" else int(valid.sum())))
    mx = x.max(1).values
    e = torch.exp(x - mx[:, None])
    se = e.sum(1)
    inv = 1.0 / se
    p = e * inv[:, None]
    py = p[rows, y]
    big = p >= F32v(CLAMP)
    q = (p * big).sum(1)
    cnt = (~big).sum(1).to(F32) + float(tile - V)                # the masked slots of the register tile hold p = 0: counted, then taken out
    if fault != "padding_counted_small":
        cnt = cnt - float(tile - V)
    bigy = py >= F32v(CLAMP)
    if fault != "label_left_in_q":
        q = torch.where(bigy, q - py, q)
        cnt = torch.where(bigy, cnt, cnt - 1.0)
    if alpha == 1.0:
        q, cnt = torch.zeros_like(q), torch.zeros_like(cnt)
    ce_rows = torch.where(valid, (mx + torch.log(se)) - x[rows, y], torch.zeros_like(mx))
    rce_rows = F32v(SCE_C) * (q + F32v(CLAMP) * cnt)
    a = torch.where(valid, F32v(alpha) / nvalid, F32v(0.0))
    bn = F32v(1.0 - alpha) / N if alpha != 1.0 else F32v(0.0)
    k_small = (a - bn * F32v(SCE_C) * q)[:, None]
    gbig = torch.zeros_like(big) if fault == "gradient_small_branch_everywhere" else big     # (Q and cnt stay right: only the multiplier)
    grad = p * torch.where(gbig, k_small + bn * F32v(SCE_C), k_small)
    grad[rows, y] = a * (py - 1.0) - bn * py * F32v(SCE_C) * q
    l_ce = ce_rows.sum() / nvalid
    loss = l_ce if alpha == 1.0 else F32v(alpha) * l_ce + F32v(1.0 - alpha) * (rce_rows.sum() / N)
    return loss, _store(grad, dtype), ce_rows, rce_rows


def _emu_adam(p, g, m, v, lr, b1, b2, eps, wd, step, fault=None):
    f = np.float32
    p, g, m, v = (z.detach().cpu().numpy().astype(f) for z in (p, g, m, v))
    lr, b1, b2, eps, wd = f(lr), f(b1), f(b2), f(eps), f(wd)
    t = f(step if fault == "t_is_step" else step + 1)
    with np.errstate(all="ignore"):
        bc1 = f(1) - f(np.power(np.float64(b1), np.float64(t)))
        bc2s = np.sqrt(f(1) - f(np.power(np.float64(b2), np.float64(t))))
        ss, decay = lr / bc1, f(1) - lr * wd
        m2 = (f(1) - b1) * (g - m) + m
        v2 = ((f(1) - b2) * g) * g + b2 * v
        upd = ss * (m2 / (np.sqrt(v2) / bc2s + eps))
        p2 = (p - upd) * decay if fault == "decay_after_step" else p * decay - upd
    p2, m2, v2 = (torch.from_numpy(np.asarray(z, dtype=f)) for z in (p2, m2, v2))
    return p2, m2, v2, p2.to(BF)


def _emu_embed_fwd(ids, table, pos, S, mask=None, dtype=F32, fault=None):
    N = ids.numel()
    t = _f(table)[ids.reshape(-1)] + _f(pos)[torch.arange(N) % S]
    return _store(t if mask is None else t * mask.to(F32), dtype)


def _emu_embed_bwd(ids, dx, V, pad_id, mask=None, fault=None):
    idf = ids.reshape(-1)
    t = _f(dx) if mask is None else _f(dx) * mask.to(F32)
    out = torch.zeros(V, t.shape[1])
    seen = {}
    for n in range(idf.numel()):                                  # increasing position order, as the kernel adds
        i = int(idf[n])
        if i == pad_id or i < 0 or i >= V:
            continue
        seen[i] = seen.get(i, 0) + 1
        if fault == "drop_one_occurrence" and seen[i] == 5 and int((idf == i).sum()) == 9:
            continue
        out[i] += t[n]
    return out


_EMU = {"ln_fwd": _emu_ln_fwd, "ln_bwd": _emu_ln_bwd, "sce": _emu_sce, "adam": _emu_adam, "embed_fwd": _emu_embed_fwd,
        "embed_bwd": _emu_embed_bwd}


# ---- shapes: the smallest at which each kernel can still go wrong ---------------------------------------------------------------------------
_LN_D = (4, 8, 252, 256, 260, 508, 512, 520, 768, 1020, 1024)
SHAPES = dict(
    ln_d={F32: _LN_D, BF: tuple(d for d in _LN_D if d % 8 == 0)},      # one lane; a full 64-lane pass +- one vector; the register-tile limit
    ln_M=(1, 3, 4, 5, 37),                                              # a partly empty last workgroup: idle waves contribute zero partials
    ln_modes=((0.0, True), (0.3, True), (0.3, False), (0.0, False)),    # (p, with res)
    ln2_d={F32: (8, 260, 1020, 1024), BF: (8, 520, 768, 1024)}, ln2_M=(1, 5, 37),
    fin_nws=(1, 31, 32, 33, 224, 225, 257, 481), fin_d=(8, 36),         # the eight-deep loop runs from 225 partial rows on
    sce_V={BF: (1, 7, 8, 9, 257, 32761, 32768, 32769, 65536), F32: (1, 3, 4, 5, 257, 16381, 16384, 16385, 32768)},
    sce_alpha=(1.0, 0.5, 0.0), sce_refused={BF: 65537, F32: 32769},
    emb_d=(4, 8, 64, 520, 768, 1024), emb_kinds=("mixed", "same", "far"), emb_p=(0.0, 0.3),
    # 8192 workgroups x 256 threads x one float4 is the largest grid of vct_adam_step_pk: the grid-stride loop takes a second trip only
    # from 8192 * 1024 + 4 elements on (256 * 4 * 1024 + 4 is one float4 past 1024 whole workgroups: a last workgroup with one thread at work)
    adam_n=(4, 1020, 1024, 1028, 256 * 4 * 1024 + 4, 8192 * 1024 + 4), adam_step=(0, 1, 999), adam_wd=(0.0, 0.01),
)
