"""fp64 reference, per-element bound, checker and a fault-injecting float32 emulation of vct_ensemble_combine (csrc/vct_ensemble.hip;
include/vct_hip.h), and the tiny models / seeds of the ensemble decode tests.  Shared by tests/test_ensemble_cpu.py (which checks THIS
file against torch.log_softmax / torch.logsumexp and shows that the checker rejects the seeded faults), tests/test_ensemble_kernel_gpu.py
and tests/test_ensemble_gpu.py.  Plain torch in float64 on whatever device the operands live on; nothing here reads the library.

Operation (written from the formulas of the header, not from the kernel's code path).  Per row and member m, inputs exactly as stored
(bf16 / fp32 -> fp64 is exact):  z = x_m[v],  M_m = max_v z,  d = z - M_m,  S_m = sum_v exp(d),  L_m = log S_m,  lp_m[v] = d - L_m.
Members with w_m == 0 are left out altogether (their rows may hold anything, NaN included).
    logp   out[v] = sum_m w_m lp_m[v]
    prob   A = max_m lp_m[v];  t_m = lp_m[v] - A;  T = sum_m w_m exp(t_m);  out[v] = A + log T   (-inf when A is -inf)
A NaN anywhere in an active member's row makes that row of out NaN.  w: the fp32 values the kernel reads, taken exactly.

Bound (tests/row_ref.py's rules: u = 2^-24 per fp32 operation, a sum of n terms in ANY order costs n u sum |terms| plus the terms'
own errors, first-order propagation; E = row_ref.SCE_EXP_ALLOW is the relative error granted to every device exp and the error
E (1 + |log|) granted to every device log; nothing is sized from the kernel's output).  M_m is exact (a maximum rounds nothing).
    d        e_d = u |d|
    exp(d)   relative E + u |d|  (the intrinsic, and the rounded argument: exp(d (1 + u)) = exp(d) (1 + u |d|))
    S        e_S = V u S + sum_v exp(d) (E + u |d|);   r_S = e_S / S
    L        e_L = 1.01 r_S + E (1 + |L|)                                  (1.01: the second-order terms of log(1 + r))
    lp       e_lp = e_d + e_L + u |lp|
    logp     e = sum_m w_m e_lp_m + (n + 1) u sum_m |w_m lp_m|              (n products, n additions, n = active members)
    prob     with q_m = w_m exp(t_m) / T (they sum to 1: d out / d lp_m = q_m):
             e = 1.01 (sum_m q_m e_lp_m + r_T) + E (1 + |log T|) + u (|A| + |log T|),
             r_T = sum_m q_m (E + 2 u |t_m|) + (n + 1) u                   (t_m rounded, then the exp's argument; n products + n additions)
    out      bound = u |out| + e + 2^-126.  Where the reference is -inf or NaN the kernel's value must be exactly that.
"""
import numpy as np
import torch

import row_ref as RR

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
U24 = RR.U24
E = RR.SCE_EXP_ALLOW
MODES = ("prob", "logp")
TINY = 2.0 ** -126

# ---- the models and seeds of tests/test_ensemble_gpu.py --------------------------------------------------------------------------------
V_TINY = 131
SEED_A, SEED_B = 5, 23                    # parameter seeds of the two members (encvar_ref.encvar_params)
# Batch seed of the greedy arg-max test.  The test ASSERTS, before it looks at any generated token, that the fp64 reference's top-2
# gap exceeds the bound above at every position of every row in both modes; tools/pick_ensemble_seed.py walks the seeds from 0 and
# prints the first for which that holds (with the smallest gap / bound ratio it saw) -- the seed recorded here.
GAP_SEED = 0


def w32(w):
    """The weights as the fp32 values the kernel reads, in fp64."""
    return [float(np.float32(x)) for x in w]


def member_logp(x):
    """(lp, e_lp) of one member's rows x [rows, V] (valid columns only), fp64."""
    z = x.to(F64)
    V = z.shape[1]
    M = z.max(1, keepdim=True).values
    d = z - M
    ex = torch.exp(d)
    S = ex.sum(1, keepdim=True)
    L = torch.log(S)
    lp = d - L
    rel_e = E + U24 * d.abs()
    e_S = V * U24 * S + torch.where(ex > 0, ex * rel_e, torch.zeros_like(ex)).sum(1, keepdim=True)
    e_L = 1.01 * e_S / S + E * (1.0 + L.abs())
    e_lp = U24 * d.abs() + e_L + U24 * lp.abs()
    return lp, e_lp


def combine(xs, w, mode):
    """(out, bound) fp64 [rows, V] of the members xs (tensors [rows, V] of fp32 / bf16) under the weights w (len(xs) floats)."""
    assert mode in MODES and len(xs) == len(w)
    w = w32(w)
    act = [(x, wm) for x, wm in zip(xs, w) if wm > 0.0]
    n = len(act)
    lps, es = zip(*(member_logp(x) for x, _ in act))
    ws = [wm for _, wm in act]
    if mode == "logp":
        out = sum(wm * lp for wm, lp in zip(ws, lps))
        e = sum(wm * e_lp for wm, e_lp in zip(ws, es)) + (n + 1) * U24 * sum((wm * lp).abs() for wm, lp in zip(ws, lps))
    else:
        stack = torch.stack(lps)
        A = stack.max(0).values
        ref = torch.where(torch.isinf(A), torch.zeros_like(A), A)
        ts = [lp - ref for lp in lps]
        terms = [wm * torch.exp(t) for wm, t in zip(ws, ts)]
        T = sum(terms)
        logT = torch.log(T)
        out = ref + logT
        out = torch.where(torch.isnan(stack).any(0), torch.full_like(out, float("nan")), out)
        qs = [term / T for term in terms]
        zero = torch.zeros_like(T)
        e_in = sum(torch.where(q > 0, q * e_lp, zero) for q, e_lp in zip(qs, es))
        r_T = sum(torch.where(q > 0, q * (E + 2 * U24 * t.abs()), zero) for q, t in zip(qs, ts)) + (n + 1) * U24
        e = 1.01 * (e_in + r_T) + E * (1.0 + logT.abs()) + U24 * (ref.abs() + logT.abs())
    bound = U24 * out.abs() + e + TINY
    return out, bound


def check(what, got, ref, bound):
    """|got - ref| <= bound wherever ref is finite; got is exactly -inf / +inf / NaN where ref is.  Prints and returns the worst
    |delta| / bound."""
    g = got.detach().to(F64)
    r, b = ref.to(g.device), bound.to(g.device)
    assert g.shape == r.shape, (tuple(g.shape), tuple(r.shape))
    fin = torch.isfinite(r)
    nan = torch.isnan(r)
    inf = ~fin & ~nan
    assert bool(torch.isnan(g[nan]).all()), f"{what}: {int((~torch.isnan(g[nan])).sum())} elements are not NaN where the reference is"
    assert bool((g[inf] == r[inf]).all()), f"{what}: {int((g[inf] != r[inf]).sum())} elements differ from the reference's infinities"
    delta = (g[fin] - r[fin]).abs()
    delta = torch.nan_to_num(delta, nan=float("inf"))
    ratio = delta / b[fin]
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print(f"[ensemble] {what}: worst |delta| / bound = {worst:.3f} over {int(fin.sum())} finite elements")
    assert worst <= 1.0, f"{what}: |delta| / bound = {worst:.3f} at finite element {int(ratio.argmax())}"
    return worst


# ---- float32 emulation with one seeded fault ----------------------------------------------------------------------------------------------
FAULTS = ("dropped_member", "unnormalised_weights", "modes_swapped", "zero_weight_not_skipped", "shifted_column")


def emulate(xs, w, mode, fault=None):
    """The operation in float32 on the CPU as a correct kernel computes it, with at most one fault of FAULTS."""
    assert fault is None or fault in FAULTS
    w = [float(np.float32(x)) for x in w]
    xs = [x.detach().cpu().to(F32) for x in xs]
    if fault == "modes_swapped":
        mode = "logp" if mode == "prob" else "prob"
    if fault == "unnormalised_weights":
        w = [2.0 * x for x in w]
    if fault == "shifted_column":
        xs = xs[:-1] + [torch.roll(xs[-1], 1, dims=1)]
    members = list(zip(xs, w))
    if fault == "dropped_member":
        members = members[:-1]
    if fault != "zero_weight_not_skipped":
        members = [(x, wm) for x, wm in members if wm > 0.0]
    lps = [torch.log_softmax(x, 1) for x, _ in members]
    ws = [torch.tensor(wm, dtype=F32) for _, wm in members]
    if mode == "logp":
        out = torch.zeros_like(lps[0])
        for wm, lp in zip(ws, lps):
            out = out + wm * lp
        return out
    stack = torch.stack(lps)
    live = torch.stack([torch.full_like(lps[0], float(wm) > 0.0, dtype=torch.bool) for wm in ws])
    A = torch.where(live, stack, torch.full_like(stack, float("-inf"))).max(0).values
    ref = torch.where(torch.isinf(A), torch.zeros_like(A), A)
    T = torch.zeros_like(A)
    for wm, lp in zip(ws, lps):
        T = T + wm * torch.exp(lp - ref)
    return ref + torch.log(T)


# ---- cases ----------------------------------------------------------------------------------------------------------------------------------
def members(rows, V, n, seed, dtypes=None, scale=3.0):
    """n members [rows, V]: random logits scale * N(0, 1), member m in dtypes[m % len(dtypes)] (default: fp32, bf16 alternating)."""
    dtypes = (F32, BF) if dtypes is None else dtypes
    return [RR.rnd((rows, V), seed + 17 * m, scale, F32).to(dtypes[m % len(dtypes)]) for m in range(n)]


def shift_case(rows, V, seed, dtypes=(F32,)):
    """Two members [rows, V >= 4]: column 0 holds +80 in the first and -80 in the second, column 1 the other way round (each member's
    own peak), column 2 holds -80 in BOTH (both log-probabilities near -160: exp underflows without the shift by A) and column 3
    -inf in both."""
    x0, x1 = members(rows, V, 2, seed, dtypes=dtypes)
    x0[:, 0], x1[:, 0] = 80.0, -80.0
    x0[:, 1], x1[:, 1] = -80.0, 80.0
    x0[:, 2] = x1[:, 2] = -80.0
    x0[:, 3] = x1[:, 3] = float("-inf")
    return x0, x1


def weights(n, seed):
    """n positive weights summing to 1 (in fp64; the kernel gets their fp32 roundings)."""
    w = np.random.default_rng(seed).uniform(0.2, 1.0, n)
    return [float(x) for x in w / w.sum()]


def tiny_models(device, dtype_a=F32, dtype_b=F32, hmme_b=False):
    """The two members of the decode tests: A (d 64 / ff 128 / 2 + 2 layers) and B (another seed, width and depth: d 32 / ff 64 /
    1 + 3 layers; hmme_b: the hierarchical encoder), two feature streams [48, 24], V 131."""
    from encvar_ref import encvar_config, encvar_params
    from helpers import build_model
    from hmm_ref import hmm_config, hmm_params
    mca = encvar_config([48, 24])
    a = build_model(mca, V_TINY, device, dtype_a, encvar_params(mca, V_TINY, SEED_A))
    if hmme_b:
        mcb = hmm_config([48, 24], [1, 2], d=32, H=4, ff=64, Ld=3)
        b = build_model(mcb, V_TINY, device, dtype_b, hmm_params(mcb, V_TINY, SEED_B))
    else:
        mcb = encvar_config([48, 24], d=32, H=4, ff=64, Le=1, Ld=3)
        b = build_model(mcb, V_TINY, device, dtype_b, encvar_params(mcb, V_TINY, SEED_B))
    return a, b


def tiny_batch(B, seed, device):
    """Two feature streams [B, 5, 48] and [B, 3, 24], no masks."""
    rng = np.random.default_rng(seed)
    return [torch.from_numpy(rng.standard_normal((B, T, Ef)).astype(np.float32)).to(device) for T, Ef in ((5, 48), (3, 24))]
