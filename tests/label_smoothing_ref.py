"""fp64 reference, derived per-element bounds, checkers and a fault-injecting float32 emulation of the label-smoothed symmetric
cross-entropy (include/vct_hip.h: vct_sce_loss_ls, csrc/vct_caption_loss.hip).  Built on tests/row_ref.py's sce() -- the un-smoothed
operation with its bounds -- which this file imports and does not change.  Shared by tests/test_label_smoothing_cpu.py (which checks
THIS file against torch.nn.functional.cross_entropy(label_smoothing=) and autograd, and shows that every checker rejects the fault
meant for it) and tests/test_label_smoothing_kernels_gpu.py.  Nothing here reads the library.

Semantics (eps = smoothing as the fp32 value the kernel receives, a = alpha / count on valid rows and 0 on pad rows)
    nll_n = lse - x[y];  smooth_n = lse - (1/V) sum_{j<V} x[j];  ce_n = (1 - eps) nll_n + eps smooth_n  (0 on pad rows)
    loss = alpha sum ce_n / count + (1 - alpha) mean_n RCE_n                                   (RCE: row_ref.sce's, never smoothed)
    grad = row_ref.sce's gradient - a eps / V in every valid column, + a eps in the label column
    stats = (sum_valid nll_n / count, #{valid n: x[y] == max_j x[j]} / count)   (a tie is a hit; a label outside [0, V) a miss)

Bounds, u = 2^-24, u_out the storage type's, every term a rounding on the kernel's path (none sized from the kernel's output):
    gradient  the kernel forms t = p_j k exactly as vct_sce_loss does -- row_ref.sce's bound without its storage term, e_t -- then
              g = t - sm with sm = fl(fl(a eps) / V), a itself one rounding: 3 u |sm|, the subtraction u |g|, storage u_out |g|.
              The label column: om = fl(1 - eps) costs a u; the chain a (p_y - om) - (RCE part) has row_ref.sce's roundings, whose
              bound 3 u a (1 + p_y) holds with om <= 1 in place of 1; then - sm as above.
    ce rows   nll and lse carry row_ref.sce's CE-row bound e_nll (lse's roundings are a subset of nll's).  sum x: every element
              passes through at most D = min(V, 64 + 6 + 16) additions (64 per thread, 6 wave steps, 16 waves): D u sum |x|;
              / V, lse - mean, eps *, om * nll (om's own rounding included) and the final sum: one u each.
    loss      row_ref.sce's composition: the rows' bounds, N u sum |rows| for the finalise's sums, 4 u |loss| for the last operations.
    stats     NLL: as the loss at alpha = 1 from the nll rows.  Accuracy: two integers below 2^24 and one division: u |acc|.
"""
import numpy as np
import torch

import row_ref as R

F64, F32, BF = R.F64, R.F32, R.BF
U24 = R.U24
SUM_DEPTH = 64 + 6 + 16


def eps32(eps):
    return float(np.float32(eps))


def sce_ls(logits, labels, alpha, eps, pad_id, dtype=F32):
    """logits [N, V] (valid columns only), labels [N] int64.  dict(loss, grad, alt, ce_rows, rce_rows, nll_rows, hit_rows, stats,
    valid, nvalid, y, a, sm, b_grad, b_ce, b_rce, b_nll, b_loss, b_stats)."""
    r = R.sce(logits, labels, alpha, pad_id, dtype)
    eps = eps32(eps)
    x = logits.to(F64)
    N, V = x.shape
    rows = torch.arange(N, device=x.device)
    lab = labels.to(x.device).reshape(-1)
    valid, y, nvalid = r["valid"], r["y"], r["nvalid"]
    oob = (lab < 0) | (lab >= V)
    one = alpha == 1.0
    beta = 0.0 if one else 1.0 - alpha
    zero = torch.zeros(N, dtype=F64, device=x.device)
    mx = x.max(1).values
    lse = mx + torch.log(torch.exp(x - mx[:, None]).sum(1))
    nll = r["ce_rows"]                                              # 0 on pad rows, NaN on a counted label outside the vocabulary
    mean = x.sum(1) / V
    smooth = lse - mean
    ce = torch.where(valid, (1.0 - eps) * nll + eps * smooth, zero)
    a = valid.to(F64) * (alpha / nvalid if nvalid else float("nan"))
    sm = a * eps / V
    grad, alt = r["grad"] - sm[:, None], r["alt"] - sm[:, None]
    grad[rows, y] += a * eps
    alt[rows, y] += a * eps
    nan = torch.tensor(float("nan"), dtype=F64, device=x.device)
    l_ce = ce.sum() / nvalid if nvalid else nan
    loss = l_ce if one else alpha * l_ce + beta * r["rce_rows"].mean()
    hit = (valid & ~oob & (x[rows, y] == mx)).to(F64)
    stats = torch.stack([nll.sum() / nvalid, hit.sum() / nvalid]) if nvalid else torch.stack([nan, nan])
    # ---- bounds
    e_t = r["b_grad"] - R.u_of(dtype) * r["grad"].abs()              # row_ref.sce's bound without its storage term
    e_g = e_t + (3 * U24 * sm.abs())[:, None] + U24 * grad.abs()
    e_g[rows, y] += a.abs() * U24
    b_grad = R.bound(grad, e_g, dtype)
    e_nll = r["b_ce"]
    depth = min(V, SUM_DEPTH)
    e_mean = depth * U24 * x.abs().sum(1) / V + U24 * mean.abs()
    om = 1.0 - eps
    e_ce = om * e_nll + eps * (e_nll + e_mean + U24 * smooth.abs()) + U24 * (eps * smooth.abs() + 2 * om * nll.abs() + ce.abs())
    e_ce = torch.where(valid, e_ce, zero)
    nv = max(nvalid, 1.0)
    el = (e_ce.nan_to_num().sum() + N * U24 * ce.abs().nan_to_num().sum()) / nv
    if not one:
        el = alpha * el + beta * (r["b_rce"].sum() + N * U24 * r["rce_rows"].sum()) / N
    b_loss = el + 4 * U24 * loss.abs()
    b_nll_mean = (e_nll.nan_to_num().sum() + N * U24 * nll.abs().nan_to_num().sum()) / nv + 2 * U24 * stats[0].abs()
    b_stats = torch.stack([b_nll_mean, U24 * stats[1].abs()])
    return dict(loss=loss, grad=grad, alt=alt, ce_rows=ce, rce_rows=r["rce_rows"], nll_rows=nll, hit_rows=hit, stats=stats, valid=valid,
                nvalid=nvalid, y=y, a=a, sm=sm, near=r["near"], b_grad=b_grad, b_ce=R.bound(ce, e_ce, F32), b_rce=r["b_rce"], b_nll=e_nll,
                b_loss=b_loss, b_stats=b_stats)


def off_label_valid(r):
    """bool [N, V]: the off-label columns of the non-pad rows."""
    m = r["valid"][:, None].expand_as(r["grad"]).clone()
    m[torch.arange(m.shape[0]), r["y"]] &= False
    return m


def share_under_half(r, bnd=None):
    """Per non-pad row: the share of off-label columns whose gradient bound lies below half of the smoothing constant a eps / V."""
    bnd = r["b_grad"] if bnd is None else bnd
    m = off_label_valid(r)
    under = (bnd < 0.5 * r["sm"][:, None]) & m
    n = m.sum(1)
    return [float(under[i].sum()) / float(n[i]) for i in range(m.shape[0]) if bool(r["valid"][i]) and int(n[i]) > 0]


# ---- checkers: what the GPU test asserts, one per property -----------------------------------------------------------------------------------
def check_loss(tag, loss, r):
    return R.check_elem(f"{tag} loss", loss.reshape(1, 1), r["loss"].reshape(1, 1), r["b_loss"].reshape(1, 1))


def check_ce_rows(tag, rows, r):
    return R.check_elem(f"{tag} CE rows", rows.reshape(1, -1), r["ce_rows"][None], r["b_ce"][None])


def check_rce_rows(tag, rows, r):
    return R.check_elem(f"{tag} RCE rows", rows.reshape(1, -1), r["rce_rows"][None], r["b_rce"][None])


def check_nll(tag, stats, r):
    return R.check_elem(f"{tag} NLL", stats.reshape(-1)[0:1].reshape(1, 1), r["stats"][0].reshape(1, 1), r["b_stats"][0].reshape(1, 1))


def check_acc(tag, stats, r):
    return R.check_elem(f"{tag} accuracy", stats.reshape(-1)[1:2].reshape(1, 1), r["stats"][1].reshape(1, 1), r["b_stats"][1].reshape(1, 1))


def check_grad(tag, dl, r):
    """Every valid column of every row against the reference (either side of the RCE clamp beside it)."""
    V = r["grad"].shape[1]
    return R.check_elem(f"{tag} gradient", dl[:, :V], r["grad"], r["b_grad"], alt=r["alt"])


def check_zeros(tag, dl, r):
    """Exact zeros on pad rows (alpha = 1: the RCE part gives every row a gradient otherwise) and in the columns behind V."""
    V = r["grad"].shape[1]
    d = dl.detach().to(F64)
    assert float(d[:, V:].abs().sum()) == 0.0, f"{tag}: the columns behind V are written as 0"
    pads = (~r["valid"]).to(d.device)
    if bool(pads.any()):
        ref0 = (r["grad"][pads.to(r["grad"].device)] == 0).to(d.device)
        got = d[pads][:, :V]
        assert bool((got[ref0] == 0).all()), f"{tag}: a pad row's gradient is not exactly 0 where the reference's is"


# ---- float32 emulation with one seeded fault ------------------------------------------------------------------------------------------------
FAULTS = {
    "eps_over_v_dropped": "gradient", "label_keeps_one": "gradient", "pad_rows_smoothed": "zeros", "mean_over_ldl": "loss",
    "padded_column_in_sum": "loss", "rce_smoothed": "rce_rows", "tie_not_a_hit": "accuracy", "nll_smoothed": "nll",
}


def emulate(logits_ld, V, labels, alpha, eps, pad_id, dtype=F32, fault=None):
    """vct_sce_loss_ls in float32 on the CPU over logits [N, ldl >= V] (the columns behind V finite here: a fault may read them).
    Returns (loss, stats [2], dlogits [N, ldl] of dtype, ce_rows, rce_rows)."""
    assert fault is None or fault in FAULTS, fault
    f = R.F32v
    xl = logits_ld.detach().to("cpu").to(F32)
    N, ldl = xl.shape
    x = xl[:, :V]
    lab = labels.reshape(-1)
    rows = torch.arange(N)
    _, g0, nll, rce = R.emulate("sce", x, lab, alpha, pad_id, dtype=F32)     # the shared part, un-smoothed, fp32 (not yet stored)
    valid = lab != pad_id
    oob = (lab < 0) | (lab >= V)
    y = torch.where(oob, torch.zeros_like(lab), lab)
    nvalid = f(float(int(valid.sum())))
    e = f(eps)
    om = f(1.0) - e
    mx = x.max(1).values
    lse = mx + torch.log(torch.exp(x - mx[:, None]).sum(1))
    sx = (xl[:, :V + 1] if fault == "padded_column_in_sum" else x).sum(1)
    mean = sx / float(ldl if fault == "mean_over_ldl" else V)
    ce = torch.where(valid, om * nll + e * (lse - mean), torch.zeros_like(nll))
    if fault == "rce_smoothed":
        rce = om * rce
    a = torch.where(valid, f(alpha) / nvalid, f(0.0))
    a_sm = f(alpha) / nvalid + torch.zeros_like(a) if fault == "pad_rows_smoothed" else a
    sm = a_sm * e / float(V)
    grad = g0.clone()
    if fault != "eps_over_v_dropped":
        grad = grad - sm[:, None]
    if fault != "label_keeps_one":
        grad[rows, y] = grad[rows, y] + a * e                     # a (p_y - 1) + a eps = a (p_y - (1 - eps)) to within the bound
    l_ce = ce.sum() / nvalid
    loss = l_ce if alpha == 1.0 else f(alpha) * l_ce + f(1.0 - alpha) * (rce.sum() / N)
    xy = x[rows, y]
    hit = valid & ~oob & (xy == mx)
    if fault == "tie_not_a_hit":
        hit = hit & ((x == mx[:, None]).sum(1) == 1)
    s0 = (ce if fault == "nll_smoothed" else nll).sum() / nvalid
    stats = torch.stack([s0, hit.to(F32).sum() / nvalid])
    dl = torch.zeros(N, ldl, dtype=F32)
    dl[:, :V] = grad
    return loss, stats, dl.to(dtype), ce, rce


def padded(x, ld, fill=float("nan")):
    """x [N, V] as the leading columns of an [N, ld] tensor of x's type whose other columns hold `fill`."""
    out = torch.full((x.shape[0], ld), fill, dtype=x.dtype, device=x.device)
    out[:, :x.shape[1]] = x
    return out


def tie_case(V, dtype):
    """(logits [2, V], ids [1, 3], pad): row 0's label sits on the LATER of two columns that share the maximum; row 1's label is not the
    maximum.  Accuracy 1/2 when the tie counts."""
    assert V >= 4
    x = R.rnd((2, V), 77, 1.0, F32)
    x[0, 1], x[0, V - 1] = 8.0, 8.0
    x[1, 0] = 8.0
    ids = torch.tensor([[0, V - 1, 2]], dtype=torch.int64)
    return x.to(dtype), ids, -1
