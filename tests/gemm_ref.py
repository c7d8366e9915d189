"""fp64 reference of the GEMM family (include/vct_hip.h: vct_gemm, vct_gemm_grouped), shared by tests/test_gemm_ref_cpu.py (which checks
THIS file against torch.nn.functional / autograd and shows that the checkers reject seeded faults) and tests/test_gemm_kernels_gpu.py.
Plain torch / numpy in float64 on whatever device the operands live on; nothing here reads the library.

Operation, in the header's own order (vct_gemm_desc, read against the epilogues in csrc/vct_gemm.hip, vct_gemm_bf16_kernel.h,
vct_gemm_pt.hip and vct_gemm_skinny.hip, which all agree):
    acc    = op(A)[M, K] op(B)[K, N]                 (valid extents only: m_valid / n_valid / k_valid inside the leading dimensions)
    x      = acc + bias[n];   preact = x             (saved BEFORE the activation, rounded to the output type)
    x      = act(x)                                  forward form, or
    x      = acc * act'(dact_src[m, n])              derivative form (no bias, no preact: the header forbids nothing, the callers never mix)
    x      = x * dropout(row * N + col)              counter computed in uint32 as in the kernels (wraps at 2^32), N = the VALID N
    C      = x + addend[m, n]                        the addend is added AFTER dropout: it is never dropped (a residual-gradient
                                                     accumulate must not be masked by the mask of the branch it joins)
    bias_grad[m] = sum_k op(A)[m, k]

Exact inputs.  ints() gives integers in [-3, 3]: every product is an integer of magnitude <= 9 and every partial sum one below
9 K <= 73 800 < 2^24 for any K used here (K <= 8200), so fp32 accumulation is exact in ANY summation order, any split, on any MFMA.
A correct kernel's fp32 output equals the reference bit for bit, its bf16 output equals Z.to(bfloat16) bit for bit (f2bf is the
hardware round-to-nearest-even, and so is torch's conversion); integer bias and addend keep that, ReLU / ReLU' too, and so does the bias
gradient (|sum| <= 3 K).

Bounds for random inputs (the formula of tests/test_layer_ss_kernels_gpu.py; none sized from the kernels under test), per element, with
u = 2^-8 for a bf16 result and 2^-24 for an fp32 one (the unit roundoff: half an ulp at the bottom of a binade), acc_term = (K + 1) 2^-24 (S + |bias|) the
worst-case fp32 accumulation error of K products and the bias in any order (S = the same product of the absolute values):
    plain / bias / addend      |got - ref| <= u |ref| + acc_term
    activation                 |got - ref| <= u |ref| + (max |act'| acc_term + 2^-20 |z|) * |dropout|      max |GELU'| = 1.13, |ReLU'| = 1
    derivative form            |got - ref| <= u |ref| + acc_term |dropout * act'(src)| + 2^-20 |acc * dropout|
    saved pre-activation       |got - ref| <= u |ref| + acc_term
The activation term: gelu_f is four fp32 roundings (x / sqrt2, 1 + erf, 0.5 x, the product) plus erff; at 4 ulp for erff that is
8 * 2^-24 = 2^-21 |z|, and the allowance is twice that -- also the figure the project grants its fast GELU' (Abramowitz-Stegun 7.1.26,
|error| <= 1.5e-7, v_exp / v_rcp at 1 ulp).  The erff figure: no math accuracy table is installed with the ROCm toolchain this was
written against (nothing under its documentation names erff), so the 4 ulp is an assumption, not a quoted figure; only the fp32
parity kernel calls erff at all -- the bf16 kernels use the polynomial above, whose absolute error 1.5e-7 / 2 |z| is 2^-23.7 |z|.  A dropout multiplier scales whatever error the element carried before it."""
import math

import numpy as np
import torch

import layer_ss_ref as LR

F64 = torch.float64
U24, U20, U8 = 2.0 ** -24, 2.0 ** -20, 2.0 ** -8
MAX_DACT = {"gelu": 1.13, "relu": 1.0, None: 1.0, "none": 1.0}


def ints(shape, seed, dtype=torch.float32, device="cpu"):
    """Integers in [-3, 3], exactly representable in bf16 and fp32."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-3, 4, tuple(shape), generator=g).to(dtype).to(device)


def rnd(shape, seed, scale=1.0, dtype=torch.float32, device="cpu"):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(tuple(shape), generator=g) * scale).to(dtype).to(device)


def _ops(a, b, ta, tb, m_valid, n_valid, k_valid):
    A = a.to(F64).t() if ta else a.to(F64)              # [M, K]
    B = b.to(F64).t() if tb else b.to(F64)              # [K, N]
    M = A.shape[0] if m_valid is None else m_valid
    N = B.shape[1] if n_valid is None else n_valid
    K = min(A.shape[1], B.shape[0]) if k_valid is None else k_valid
    return A[:M, :K], B[:K, :N]


def product(a, b, ta=False, tb=True, m_valid=None, n_valid=None, k_valid=None):
    """(Z, S): the fp64 product of the valid extents and the same product of the absolute values."""
    A, B = _ops(a, b, ta, tb, m_valid, n_valid, k_valid)
    return A @ B, A.abs() @ B.abs()


def bias_grad(a, ta=True, m_valid=None, k_valid=None):
    """sum over K of op(A): [M] (db = the column sums of dY for ta = 1)."""
    A = a.to(F64).t() if ta else a.to(F64)
    M = A.shape[0] if m_valid is None else m_valid
    K = A.shape[1] if k_valid is None else k_valid
    return A[:M, :K].sum(dim=1)


def act_fn(name, x):
    if name == "gelu":
        return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))
    return torch.clamp(x, min=0.0) if name == "relu" else x


def dact_fn(name, x):
    if name == "gelu":
        return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    return (x > 0).to(x.dtype) if name == "relu" else torch.ones_like(x)


def drop_mask(M, N, drop, device="cpu"):
    """Multipliers [M, N] (0 or 1 / (1 - p) as fp32) of dropout = (seed, site, p); idx = row * N + col in uint32."""
    if drop is None or drop[2] <= 0.0:
        return torch.ones(M, N, dtype=F64, device=device)
    seed, site, p = drop
    idx = (np.arange(M, dtype=np.uint64)[:, None] * np.uint64(N) + np.arange(N, dtype=np.uint64)[None]) & np.uint64(0xFFFFFFFF)
    return torch.from_numpy(LR.drop_mult(int(seed), int(site), float(p), idx)).to(F64).to(device)


def epilogue(Z, bias=None, act=None, addend=None, dact_src=None, drop=None):
    """dict(out, preact, z, mask, dact): the header's order -- bias, activation (preact saved before it) or acc * act'(dact_src),
    dropout on C, then the addend."""
    M, N = Z.shape
    z = Z if bias is None else Z + bias.to(F64)[:N]
    mask = drop_mask(M, N, drop, Z.device)
    d = None
    if dact_src is not None:
        d = dact_fn(act, dact_src.to(F64)[:M, :N])
        x = z * d
    else:
        x = act_fn(act, z)
    x = x * mask
    if addend is not None:
        x = x + addend.to(F64)[:M, :N]
    return dict(out=x, preact=z, z=z, mask=mask, dact=d)


def bound(ref, S, K, out_dtype, bias=None, act=None, e=None, what="out"):
    """Per-element bound of the module docstring.  e = epilogue()'s dict (needed with an activation, a derivative or dropout)."""
    u = U8 if out_dtype == torch.bfloat16 else U24
    acc = (K + 1) * U24 * (S if bias is None else S + bias.to(F64)[:S.shape[1]].abs())
    if what == "preact" or e is None:
        return u * ref.abs() + acc
    mask = e["mask"].abs()
    if e["dact"] is not None:
        return u * ref.abs() + acc * (mask * e["dact"]).abs() + U20 * (e["z"] * mask).abs()
    if act in ("gelu", "relu"):
        return u * ref.abs() + (MAX_DACT[act] * acc + U20 * e["z"].abs()) * mask
    return u * ref.abs() + acc * mask


def _c(t, like=None):
    """fp64 copy on the device of `like` (the checkers run where the kernel's output lives: no host copy of a large output)."""
    return t.detach().to(F64) if like is None else t.detach().to(like.device).to(F64)


def _worst(x):
    w = int(x.argmax())
    return (w // x.shape[1], w % x.shape[1]) if x.dim() == 2 else (w, 0)


def check_exact(what, got, ref, out_dtype=None):
    """Bit for bit: ref (fp64, exactly representable in fp32) rounded to the output type must equal got."""
    out_dtype = got.dtype if out_dtype is None else out_dtype
    g, r = _c(got), _c(ref.to(torch.float32).to(out_dtype), got)
    if g.dim() == 1:
        g, r = g[:, None], r[:, None]
    bad = ~((g == r) | (torch.isnan(g) & torch.isnan(r)))
    bad |= torch.isnan(g)
    n = int(bad.sum())
    diff = torch.where(bad, torch.nan_to_num((g - r).abs(), nan=float("inf")), torch.zeros_like(g))
    r0, c0 = _worst(diff)
    print(f"[gemm] {what}: exact, {n} of {g.numel()} elements differ; worst |delta| = {float(diff.max()):.3e} at row {r0} column {c0}")
    assert n == 0, f"{what}: {n} elements differ, worst at row {r0} column {c0}: got {float(g[r0, c0])!r}, reference {float(r[r0, c0])!r}"


def check_elem(what, got, ref, bnd):
    """|got - ref| <= bnd at every element; prints the worst excess.  Returns it."""
    g, r, b = _c(got), _c(ref, got), _c(bnd, got)
    if g.dim() == 1:
        g, r, b = g[:, None], r[:, None], b[:, None]
    excess = torch.nan_to_num((g - r).abs() - b, nan=float("inf"))
    r0, c0 = _worst(excess)
    ratio = float(((g - r).abs() / b.clamp(min=1e-300)).nan_to_num(nan=float("inf")).max())
    print(f"[gemm] {what}: worst |delta| - bound = {float(excess.max()):.3e} at row {r0} column {c0} (worst |delta| / bound = {ratio:.3f})")
    assert float(excess.max()) <= 0.0, (f"{what}: row {r0} column {c0}: got {float(g[r0, c0])!r}, reference {float(r[r0, c0])!r}, "
                                        f"bound {float(b[r0, c0]):.3e}")
    return ratio


def check_mask(what, got, ref, tiny=None):
    """The elements zero in one tensor and not in the other must number 0.  tiny: elements whose exact value lies below the documented
    absolute error of the fast GELU (gelu_tiny: the kernel may hold -0 there); they are counted, printed and left out."""
    a, b = _c(got) == 0, _c(ref, got) == 0
    bad = a != b
    if tiny is not None:
        tiny = tiny.to(bad.device)
        print(f"[gemm] {what}: {int((tiny & ~b).sum())} non-zero reference elements below the activation's absolute error, "
              f"{int((tiny & bad).sum())} of them 0 in the kernel")
        bad = bad & ~tiny
    n = int(bad.sum())
    print(f"[gemm] {what}: {int(b.sum())} zeros in the reference, {n} mismatches")
    assert n == 0, f"{what}: {n} elements zero in one and not in the other, first at (row, column) {bad.nonzero()[0].tolist()}"


def gelu_tiny(z):
    """The fast GELU (csrc/vct_common.h: erf by Abramowitz-Stegun 7.1.26, |error| <= 1.5e-7, evaluated in fp32 as 1 - poly * e, which is
    1 exactly once poly * e < 2^-25) has an absolute error of up to |z| (0.75e-7 + 2^-25) < 2^-22 |z|: below about z = -5 the exact
    value z Phi(z) is smaller than that and the kernel's result is -0.  Those elements (and only those) may be zero in the kernel."""
    return (act_fn("gelu", z).abs() <= 2.0 ** -22 * z.abs()) & (z != 0)


# ---- a correct emulation of the kernels' arithmetic (CPU) and the seeded faults the checkers must reject -----------------------------------
FAULTS = ("drop_k_element", "drop_k_tile_block", "swap_rows", "shift_cols", "shift_bias", "double_partial", "truncate_bf16")


def emulate(a, b, ta=False, tb=True, m_valid=None, n_valid=None, k_valid=None, bias=None, act=None, addend=None, dact_src=None,
            drop=None, out_dtype=torch.bfloat16, split=3, seed=0, fault=None):
    """What a correct kernel computes, on the CPU: operands as given (bf16 or fp32 values), fp32 accumulation in K tiles of 64 (each
    tile's products summed in fp32), the tiles dealt to `split` partials that are summed in a shuffled order, the epilogue in fp32, the
    result rounded to out_dtype.  fault: one of FAULTS, applied at a pseudo-random place."""
    A, B = _ops(a.to("cpu"), b.to("cpu"), ta, tb, m_valid, n_valid, k_valid)
    A, B = A.to(torch.float32).clone(), B.to(torch.float32)
    M, K = A.shape
    N = B.shape[1]
    rs = np.random.RandomState(seed)
    nkt = (K + 63) // 64
    split = max(1, min(split, nkt))
    per = (nkt + split - 1) // split
    if fault == "drop_k_element":
        # one k element of one output row never reaches the accumulator (the largest operand of that row: any element would do for
        # the exact check, the bound check needs one that matters)
        r = int(rs.randint(M))
        A[r, int(A[r].abs().argmax())] = 0.0
    parts = []
    blk = (int(rs.randint((M + 15) // 16)), int(rs.randint((N + 15) // 16)), int(rs.randint(nkt)))
    for z in range(split):
        acc = torch.zeros(M, N, dtype=torch.float32)
        for kt in range(z * per, min(nkt, (z + 1) * per)):
            t = A[:, kt * 64:(kt + 1) * 64] @ B[kt * 64:(kt + 1) * 64]
            if fault == "drop_k_tile_block" and kt == blk[2]:
                t[blk[0] * 16:(blk[0] + 1) * 16, blk[1] * 16:(blk[1] + 1) * 16] = 0.0
            acc = acc + t
        parts.append(acc)
    if fault == "double_partial":
        parts.append(parts[int(rs.randint(len(parts)))].clone())
    order = rs.permutation(len(parts))
    acc = torch.zeros(M, N, dtype=torch.float32)
    for i in order:
        acc = acc + parts[int(i)]
    f32 = lambda t: None if t is None else t.to("cpu").to(torch.float32)
    bv = f32(bias)
    if bv is not None:
        bv = bv[:N]
        if fault == "shift_bias":
            bv = torch.roll(bv, 1)
        acc = acc + bv
    pre = acc
    if dact_src is not None:
        x = acc * dact_fn(act, f32(dact_src)[:M, :N])
    else:
        x = act_fn(act, acc)
    x = x * drop_mask(M, N, drop).to(torch.float32)
    if addend is not None:
        x = x + f32(addend)[:M, :N]
    if fault == "swap_rows":
        r = int(rs.randint(max(M - 1, 1)))
        x = x.clone()
        x[[r, min(r + 1, M - 1)]] = x[[min(r + 1, M - 1), r]]
    if fault == "shift_cols":
        x = torch.roll(x, 1, dims=1)
    if fault == "truncate_bf16" and out_dtype == torch.bfloat16:
        out = (x.contiguous().view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)      # chop instead of round
    else:
        out = x.to(out_dtype)
    return out, pre.to(out_dtype)


# ---- the shapes of tests/test_gemm_kernels_gpu.py (shared with the CPU test, which runs the emulation at every one of them) -------------------
TILES = {1: (128, 128), 2: (128, 64), 3: (64, 128), 4: (64, 64), 5: (128, 128), 8: (128, 64), 6: (256, 128), 7: (320, 128), 9: (64, 128)}
VARIANT = {1: 0, 2: 0, 3: 0, 4: 0, 5: 1, 8: 4, 6: 6, 7: 7, 9: 9}       # the eight-wave variant id of a tile code
GENERAL_K = (8, 64, 72, 192, 200, 203)
SPLIT_K = (1000, 1032)
F32_K = (4, 16, 20, 52)
SKINNY_M, SKINNY_N, SKINNY_K = (1, 15, 16, 17, 256), (16, 17, 4096), (64, 72, 8192)
PT_M, PT_K = (1024, 1025, 1151), (128, 136, 4096)
G256 = {"nt": (2049, 8200, 264), "nt_splitk": (2049, 200, 8200), "nn": (300, 264, 8200), "tn": (3845, 3100, 2056)}
GROUP_MN = ((200, 72), (1, 8), (64, 64), (65, 136), (136, 65), (129, 24), (77, 264), (256, 128))
GROUP_ROWS = (8, 328, 1000, 1003)


def general_mn(bm, bn):
    return ((1, 1), (bm - 1, bn + 1), (bm + 1, bn - 1), (2 * bm + 3, 8))


def gpu_file_shapes():
    """Every (M, N, K) the GPU file runs, once."""
    s = set()
    for bm, bn in set(TILES.values()):
        for m, n in general_mn(bm, bn) + ((bm + 1, 77),):
            s |= {(m, n, k) for k in GENERAL_K}
    s |= {(m, n, k) for (m, n) in ((130, 72), (65, 77), (1, 72), (7, 72), (16, 72), (1024, 1024)) for k in SPLIT_K}
    s |= {(m, n, k) for (m, n) in general_mn(64, 64) + ((2049, 3080),) for k in F32_K}
    s |= {(m, n, k) for m in SKINNY_M + (257,) for n in SKINNY_N + (15,) for k in SKINNY_K + (56, 76)}
    s |= {(m, n, k) for m in PT_M for n in (1032, 256) for k in PT_K}
    s |= set(G256.values())
    s |= {(m, n, k) for (m, n) in GROUP_MN for k in GROUP_ROWS}
    return sorted(s)
