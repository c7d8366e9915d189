"""Kernel-level tests (GPU) of the memory-bound row kernels -- vct_add_ln_fwd / _bwd, vct_add_ln_ln_fwd / _bwd,
vct_ln_param_finalize_batched, vct_sce_loss, vct_embed_fwd / vct_embed_bwd_live and vct_adam_step -- through vct_amd.ops only, every
element against the fp64 reference of the same operation and the derived per-element bounds of tests/row_ref.py (itself checked by
tests/test_row_ref_cpu.py, which also shows that each checker used here rejects the faults of row_ref.FAULTS).

Harness.  Outputs live in an Arena (tests/gpu_arena.py) filled with 0xFF, 64 canary bytes on both sides of each.  Operands carry NaN
wherever a kernel must not read, or where the value must not reach an output: the rows behind M (N, n) of every operand, the columns
V .. ldl of the logits, the table rows of ids that do not occur in an embedding forward, the dx rows of pad positions and of ids outside
the table in the embedding backward (the header gives them no row: "row pad_id zero", "an id outside [0, V) owns no row"), and every
workspace on entry (param_ws, row_ws; the embedding's integer workspace holds -1).  The pad id's TABLE row stays finite: the forward
reads it like any other.  Every call runs twice on fresh arenas: the two arenas must be byte-identical, every valid output finite, every
canary intact.  Dropout masks come from layer_ss_ref.drop_mult (row_ref.drop_mask) and are compared exactly; none is read off a kernel.

One pytest case per kernel and type, the shapes of row_ref.SHAPES looped inside; each prints the worst |delta| / bound it met."""
import pytest
import torch

import row_ref as R
from gpu_arena import Arena, up

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64, F32, BF = R.F64, R.F32, R.BF
NAN = float("nan")
S = R.SHAPES
TYPES = pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
SEED, SITE = 1234, 5


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from vct_amd import ops as _ops
    return _ops


def guard(vals, extra=2):
    """vals [R, C] (or [n]) as the leading part of a buffer with `extra` more rows (8 more elements) of NaN behind it."""
    v = vals.to(DEV)
    if v.dim() == 1:
        buf = torch.full((v.numel() + 8,), NAN, dtype=v.dtype, device=DEV)
        buf[:v.numel()] = v
        return buf[:v.numel()]
    buf = torch.full((v.shape[0] + extra, v.shape[1]), NAN, dtype=v.dtype, device=DEV)
    buf[:v.shape[0]] = v
    return buf[:v.shape[0]]


def vec(name, n, dtype=F32):
    return (name, 1, n, dtype, n, 0)


def mat(name, rows, cols, dtype, ld=None):
    return (name, rows, cols, dtype, cols if ld is None else ld, 0)


def twice(build, nonfinite_ok=()):
    """build() -> (arena, extra): run on two fresh arenas; byte-identical, canaries intact, outputs finite.  Returns the first."""
    a1, x1 = build()
    a2, _ = build()
    torch.cuda.synchronize()
    assert torch.equal(a1.buf, a2.buf), "two runs on fresh arenas differ"
    a1.check(nonfinite_ok)
    a2.check(nonfinite_ok)
    return a1, x1


def drop_of(p):
    """(the ops' dropout triple, the reference's)"""
    if p <= 0.0:
        return None, None
    return (torch.tensor([SEED], dtype=torch.int32, device=DEV), SITE, p), (SEED, SITE, p)


def report(capsys, what, worst):
    capsys.readouterr()
    with capsys.disabled():
        print(f"\n[row] {what}: kernels, worst |delta| / bound = {worst:.3f}")
    assert worst <= 1.0


# ---- LayerNorm ------------------------------------------------------------------------------------------------------------------------------
def ln_case(M, d, dtype, p, with_res, seed):
    x, res = R.ln_rows(M, d, seed, dtype, with_res, DEV)
    gamma, beta = R.ln_params(d, seed + 5, DEV)
    dy = R.rnd((M, d), seed + 7, 1.0, dtype, DEV)
    dk, dr = drop_of(p)
    mask = R.drop_mask(M, d, dr, DEV) if dr else None
    return x, res, gamma, beta, dy, dk, mask


def run_ln_fwd(ops, tag, dtype, x, res, gamma, beta, dk, mask):
    M, d = x.shape
    xg, rg = guard(x), (None if res is None else guard(res))

    def build():
        a = Arena([mat("y", M, d, dtype), vec("mean", M), vec("rstd", M)])
        ops.add_ln_fwd(xg, rg, gamma, beta, a["y"], a["mean"], a["rstd"], dropout=dk)
        return a, None
    a, _ = twice(build)
    f = R.ln_fwd(x, res, gamma, beta, mask)
    w = [R.check_elem(f"{tag} y", a["y"], f["y"], R.bound(f["y"], f["e_y"], dtype)),
         R.check_elem(f"{tag} mean", a["mean"], f["mean"], R.bound(f["mean"], f["e_mean"], F32)),
         R.check_elem(f"{tag} rstd", a["rstd"], f["rstd"], R.bound(f["rstd"], f["e_rstd"], F32))]
    return max(w), f


def run_ln_bwd(ops, tag, dtype, x, res, gamma, dy, f, dk, mask, with_dxo=True, defer=False):
    """add_ln_bwd on the reference's statistics rounded to fp32 (the backward's operands).  defer: dgamma / dbeta left to
    ln_param_finalize_batched (one table entry)."""
    M, d = x.shape
    nws = ops.ln_ws_rows(M)
    assert nws == (M + 3) // 4
    xg, rg, dyg = guard(x), (None if res is None else guard(res)), guard(dy)
    mean, rstd = guard(f["mean"].to(F32)), guard(f["rstd"].to(F32))

    def build():
        a = Arena([mat("ds", M, d, dtype), mat("dxo", M, d, dtype), vec("dgamma", d), vec("dbeta", d), mat("ws", 2 * nws, d, F32)])
        dxo = a["dxo"] if with_dxo else None
        if defer:
            ops.add_ln_bwd(dyg, xg, rg, gamma, mean, rstd, a["ds"], dxo, None, None, a["ws"], dropout=dk)
            table = torch.tensor([[a["ws"].data_ptr(), a["dgamma"].data_ptr(), a["dbeta"].data_ptr(), nws]], dtype=torch.int64, device=DEV)
            ops.ln_param_finalize_batched(table, 1, d)
        else:
            ops.add_ln_bwd(dyg, xg, rg, gamma, mean, rstd, a["ds"], dxo, a["dgamma"], a["dbeta"], a["ws"], dropout=dk)
        if not with_dxo:
            a["dxo"].zero_()
        return a, None
    a, _ = twice(build)
    b = R.ln_bwd(dy, x, res, gamma, mean, rstd, mask)
    w = [R.check_elem(f"{tag} ds", a["ds"], b["ds"], R.bound(b["ds"], b["e_ds"], dtype)),
         R.check_elem(f"{tag} dgamma", a["dgamma"], b["dgamma"], R.bound(b["dgamma"], b["e_dgamma"], F32)),
         R.check_elem(f"{tag} dbeta", a["dbeta"], b["dbeta"], R.bound(b["dbeta"], b["e_dbeta"], F32))]
    if with_dxo:
        bd = R.bound(b["dxo"], b["e_dxo"], dtype)
        w.append(R.check_elem(f"{tag} dxo", a["dxo"], b["dxo"], bd))
        if mask is not None:
            R.check_mask(f"{tag} dxo mask", a["dxo"], b["dxo"], bd)
    # the partial rows: their column sums are dgamma | dbeta too (any order of nws rows is inside the M-term bound)
    ws = a["ws"].view(nws, 2, d).double().sum(0)
    w += [R.check_elem(f"{tag} ws dgamma", ws[0], b["dgamma"], R.bound(b["dgamma"], b["e_dgamma"], F32)),
          R.check_elem(f"{tag} ws dbeta", ws[1], b["dbeta"], R.bound(b["dbeta"], b["e_dbeta"], F32))]
    return max(w)


@TYPES
def test_add_ln_fwd_bwd(ops, dtype, capsys):
    """vct_add_ln_fwd / vct_add_ln_bwd (with its own finalize kernel): y, mean, rstd, ds, dxo, dgamma, dbeta, the partial rows."""
    worst = 0.0
    for d in S["ln_d"][dtype]:
        for M in S["ln_M"]:
            for i, (p, with_res) in enumerate(S["ln_modes"]):
                tag = f"ln {M}x{d} p={p} res={with_res}"
                x, res, gamma, beta, dy, dk, mask = ln_case(M, d, dtype, p, with_res, 100 + d + M + i)
                wf, f = run_ln_fwd(ops, tag, dtype, x, res, gamma, beta, dk, mask)
                # dxo may be NULL when res == NULL and p == 0: that form runs without it
                wb = run_ln_bwd(ops, tag, dtype, x, res, gamma, dy, f, dk, mask, with_dxo=not (p == 0.0 and not with_res))
                worst = max(worst, wf, wb)
    report(capsys, f"add_ln_fwd / add_ln_bwd {dtype}", worst)


@TYPES
def test_add_ln_ln_fwd_bwd(ops, dtype, capsys):
    """The two-norm forms against fp64 (not against two launches of the same code): the second norm on y as stored, the backward's
    gradient of y rounded to the storage type (its bound enters the layer norm's as dy_err), both parameter gradients through
    ln_param_finalize_batched with a table of two."""
    worst = 0.0
    for d in S["ln2_d"][dtype]:
        for M in S["ln2_M"]:
            for p in (0.0, 0.3):
                tag = f"ln-ln {M}x{d} p={p}"
                x, res, gamma, beta, dy2, dk, mask = ln_case(M, d, dtype, p, True, 500 + d + M)
                gamma2, beta2 = R.ln_params(d, 900 + d, DEV)
                xg, rg = guard(x), guard(res)

                def build_f():
                    a = Arena([mat("y", M, d, dtype), vec("mean", M), vec("rstd", M), mat("y2", M, d, dtype), vec("mean2", M), vec("rstd2", M)])
                    ops.add_ln_ln_fwd(xg, rg, gamma, beta, a["y"], a["mean"], a["rstd"], gamma2, beta2, a["y2"], a["mean2"], a["rstd2"], dropout=dk)
                    return a, None
                a, _ = twice(build_f)
                f = R.ln_fwd(x, res, gamma, beta, mask)
                f2 = R.ln_fwd(a["y"], None, gamma2, beta2)                  # built on the rows the kernel stored
                w = [R.check_elem(f"{tag} y", a["y"], f["y"], R.bound(f["y"], f["e_y"], dtype)),
                     R.check_elem(f"{tag} mean", a["mean"], f["mean"], R.bound(f["mean"], f["e_mean"], F32)),
                     R.check_elem(f"{tag} rstd", a["rstd"], f["rstd"], R.bound(f["rstd"], f["e_rstd"], F32)),
                     R.check_elem(f"{tag} y2", a["y2"], f2["y"], R.bound(f2["y"], f2["e_y"], dtype)),
                     R.check_elem(f"{tag} mean2", a["mean2"], f2["mean"], R.bound(f2["mean"], f2["e_mean"], F32)),
                     R.check_elem(f"{tag} rstd2", a["rstd2"], f2["rstd"], R.bound(f2["rstd"], f2["e_rstd"], F32))]
                # backward: operands made by the reference (y as stored = the fp64 y rounded to the storage type)
                y_st = R.to_storage(f["y"], dtype).to(dtype)
                s2 = R.ln_fwd(y_st, None, gamma2, beta2)
                nws = ops.ln_ws_rows(M)
                yg, dyg = guard(y_st), guard(dy2)
                mean, rstd, mean2, rstd2 = (guard(t.to(F32)) for t in (f["mean"], f["rstd"], s2["mean"], s2["rstd"]))

                def build_b():
                    b = Arena([mat("ds", M, d, dtype), mat("dxo", M, d, dtype), vec("dgamma", d), vec("dbeta", d), vec("dgamma2", d),
                               vec("dbeta2", d), mat("ws", 2 * nws, d, F32), mat("ws2", 2 * nws, d, F32)])
                    ops.add_ln_ln_bwd(dyg, yg, gamma2, mean2, rstd2, b["ws2"], xg, rg, gamma, mean, rstd, b["ds"], b["dxo"], b["ws"], dropout=dk)
                    table = torch.tensor([[b["ws2"].data_ptr(), b["dgamma2"].data_ptr(), b["dbeta2"].data_ptr(), nws],
                                          [b["ws"].data_ptr(), b["dgamma"].data_ptr(), b["dbeta"].data_ptr(), nws]], dtype=torch.int64, device=DEV)
                    ops.ln_param_finalize_batched(table, 2, d)
                    return b, None
                b, _ = twice(build_b)
                front = R.ln_bwd(dy2, y_st, None, gamma2, mean2, rstd2)
                dy_err = R.bound(front["ds"], front["e_ds"], dtype)
                back = R.ln_bwd(R.to_storage(front["ds"], dtype), x, res, gamma, mean, rstd, mask, dy_err=dy_err)
                bd = R.bound(back["dxo"], back["e_dxo"], dtype)
                w += [R.check_elem(f"{tag} ds", b["ds"], back["ds"], R.bound(back["ds"], back["e_ds"], dtype)),
                      R.check_elem(f"{tag} dxo", b["dxo"], back["dxo"], bd),
                      R.check_elem(f"{tag} dgamma", b["dgamma"], back["dgamma"], R.bound(back["dgamma"], back["e_dgamma"], F32)),
                      R.check_elem(f"{tag} dbeta", b["dbeta"], back["dbeta"], R.bound(back["dbeta"], back["e_dbeta"], F32)),
                      R.check_elem(f"{tag} dgamma2", b["dgamma2"], front["dgamma"], R.bound(front["dgamma"], front["e_dgamma"], F32)),
                      R.check_elem(f"{tag} dbeta2", b["dbeta2"], front["dbeta"], R.bound(front["dbeta"], front["e_dbeta"], F32))]
                if mask is not None:
                    R.check_mask(f"{tag} dxo mask", b["dxo"], back["dxo"], bd)
                worst = max(worst, max(w))
    report(capsys, f"add_ln_ln_fwd / add_ln_ln_bwd {dtype}", worst)


def test_ln_param_finalize_batched_through_the_backward(ops, capsys):
    """M = 4 nws rows (and one M = 4 nws - 3) with dgamma / dbeta deferred: from 225 partial rows on the eight-loads-in-flight loop runs."""
    worst = 0.0
    for d in S["fin_d"]:
        for nws in S["fin_nws"]:
            for M in (4 * nws,) + ((4 * nws - 3,) if nws == 481 else ()):
                for dtype in (F32, BF) if (d % 8 == 0 and nws in (33, 225)) else (F32,):
                    x, res, gamma, beta, dy, dk, mask = ln_case(M, d, dtype, 0.0, True, 700 + nws + d)
                    f = R.ln_fwd(x, res, gamma, beta, mask)
                    worst = max(worst, run_ln_bwd(ops, f"finalize M={M} d={d}", dtype, x, res, gamma, dy, f, dk, mask, defer=True))
    report(capsys, "ln_param_finalize_batched behind add_ln_bwd", worst)


def test_ln_param_finalize_batched_exact_column_sums(ops):
    """Hand-filled partial rows of small integers (exact in any order), a table of three entries with different row counts; d = 36 puts
    the gamma | beta seam inside a 32-column workgroup and leaves the last one ragged.  NaN in the rows behind each entry's count."""
    for d in S["fin_d"]:
        for counts in ((1, 31, 32), (33, 224, 225), (257, 481, 225)):
            wss = [torch.full((nws + 2, 2, d), NAN, device=DEV) for nws in counts]
            for i, (w, nws) in enumerate(zip(wss, counts)):
                w[:nws] = R.G.ints((nws, 2, d), 40 + i + nws, F32, DEV)

            def build():
                a = Arena([vec(f"{k}{i}", d) for i in range(3) for k in ("dgamma", "dbeta")])
                table = torch.tensor([[w.data_ptr(), a[f"dgamma{i}"].data_ptr(), a[f"dbeta{i}"].data_ptr(), n]
                                      for i, (w, n) in enumerate(zip(wss, counts))], dtype=torch.int64, device=DEV)
                ops.ln_param_finalize_batched(table, 3, d)
                return a, None
            a, _ = twice(build)
            for i, (w, nws) in enumerate(zip(wss, counts)):
                sums = w[:nws].double().sum(0)
                R.check_exact(f"finalize d={d} rows={nws} dgamma", a[f"dgamma{i}"], sums[0][None])
                R.check_exact(f"finalize d={d} rows={nws} dbeta", a[f"dbeta{i}"], sums[1][None])


# ---- symmetric cross-entropy ---------------------------------------------------------------------------------------------------------------
def sce_run(ops, dtype, V, alpha, form, x, ids, pad, ld_dl=None):
    """One form of the call on a fresh arena: 'separate', 'inplace', 'wide' (ld_dl given) or 'forward'."""
    v = R.vec_of(dtype)
    N, vr, limit = x.shape[0], up(V, v), 8192 * v
    labels = ids[:, 1:]
    specs = [vec("loss", 1), ("row_ws", 1, 2 * N + 1, F32, 2 * N + 2, 0)]
    if form == "inplace":
        a = Arena(specs + [mat("dl", N, vr, dtype)])
        a["dl"][:, :V] = x
        logits = dl = a["dl"]
    else:
        ldl = min(vr + v, limit)
        buf = torch.full((N + 1, ldl), NAN, dtype=dtype, device=DEV)
        buf[:N, :V] = x
        logits = buf[:N]
        if form == "forward":
            a, dl = Arena(specs), None
        else:
            w = vr if ld_dl is None else ld_dl
            a = Arena(specs + [mat("dl", N, w, dtype)])
            dl = a["dl"]
    ops.sce_loss(logits, V, labels, labels.shape[1], pad, alpha, a["loss"], dl, a["row_ws"])
    return a


def sce_check(tag, a, r, V, alpha, N, grad=True):
    w = [R.check_elem(f"{tag} loss", a["loss"], r["loss"].reshape(1, 1), r["b_loss"].reshape(1, 1)),
         R.check_elem(f"{tag} CE rows", a["row_ws"][:, :N], r["ce_rows"][None], r["b_ce"][None])]
    if alpha != 1.0:
        w.append(R.check_elem(f"{tag} RCE rows", a["row_ws"][:, N:2 * N], r["rce_rows"][None], r["b_rce"][None]))
    assert float(a["row_ws"][0, 2 * N]) == r["nvalid"], "count of valid rows"
    if grad:
        w.append(R.check_elem(f"{tag} gradient", a["dl"][:, :V], r["grad"], r["b_grad"], alt=r["alt"]))
        assert float(a["dl"][:, V:].abs().sum()) == 0.0, f"{tag}: the columns behind V are written as 0"
    return max(w)


@TYPES
def test_sce_loss(ops, dtype, capsys):
    """vct_sce_loss: every V of row_ref.SHAPES x alpha x the four forms.  In place and separate share a route and must agree bit for bit
    (loss and gradient), the forward-only loss with them, and so must the wider ld_dl wherever it stays in the same instantiation
    (row_ref.sce_tile); where it takes the other route it is judged against fp64 alone."""
    worst, routes = 0.0, set()
    v = R.vec_of(dtype)
    for V in S["sce_V"][dtype]:
        for alpha in S["sce_alpha"]:
            x, ids, pad = R.sce_case(V, 40, dtype)
            x, ids = x.to(DEV), ids.to(DEV)
            N = x.shape[0]
            r = R.sce(x, ids[:, 1:].reshape(-1), alpha, pad, dtype)
            vr = up(V, v)
            wide = min(vr + v, 8192 * v)
            got = {}
            for form in ("separate", "inplace", "forward") + (("wide",) if wide > vr else ()):
                ld = wide if form == "wide" else None
                a, _ = twice(lambda: (sce_run(ops, dtype, V, alpha, form, x, ids, pad, ld), None))
                worst = max(worst, sce_check(f"sce V={V} alpha={alpha} {form}", a, r, V, alpha, N, grad=form != "forward"))
                routes.add(R.sce_tile(V, 0 if form == "forward" else (wide if form == "wide" else vr), dtype)[1])
                got[form] = a
            assert torch.equal(got["separate"]["dl"], got["inplace"]["dl"]), (V, alpha, "in place differs from separate")
            same = ["inplace", "forward"]
            if "wide" in got and R.sce_tile(V, wide, dtype) == R.sce_tile(V, vr, dtype):
                # the wider ld_dl stays in the same instantiation: the same definition, so the same bits in the valid columns
                same.append("wide")
                assert torch.equal(got["separate"]["dl"][:, :V], got["wide"]["dl"][:, :V]), (V, alpha, "wide ld_dl differs from separate")
            for form in same:
                assert torch.equal(got["separate"]["loss"], got[form]["loss"]), (V, alpha, form)
                assert torch.equal(got["separate"]["row_ws"], got[form]["row_ws"]), (V, alpha, form)
    # a small V whose ld_dl alone selects the wide-row instantiation
    for alpha in (0.5, 1.0):
        V = 257
        x, ids, pad = R.sce_case(V, 41, dtype)
        x, ids = x.to(DEV), ids.to(DEV)
        r = R.sce(x, ids[:, 1:].reshape(-1), alpha, pad, dtype)
        ld = 4096 * v + v
        a, _ = twice(lambda: (sce_run(ops, dtype, V, alpha, "wide", x, ids, pad, ld), None))
        worst = max(worst, sce_check(f"sce V={V} alpha={alpha} ld_dl={ld}", a, r, V, alpha, x.shape[0]))
        routes.add(R.sce_tile(V, ld, dtype)[1])
    assert len(routes) == 2, routes
    capsys.readouterr()
    with capsys.disabled():
        print(f"\n[row] sce_loss instantiations reached: {sorted(routes)}")
    report(capsys, f"sce_loss {dtype}", worst)


@TYPES
def test_sce_loss_label_outside_the_vocabulary(ops, dtype):
    """A label equal to V where ldl > V: the documented result is a NaN loss, nothing written outside the row (canaries, the padding of
    row_ws) and finite gradients -- the row itself is computed against column 0, as the reference does."""
    V, alpha = 257, 0.5
    x, ids, pad = R.sce_case(V, 42, dtype, oob=True)
    x, ids = x.to(DEV), ids.to(DEV)
    r = R.sce(x, ids[:, 1:].reshape(-1), alpha, pad, dtype)
    a, _ = twice(lambda: (sce_run(ops, dtype, V, alpha, "separate", x, ids, pad), None), nonfinite_ok=("loss", "row_ws"))
    assert bool(torch.isnan(a["loss"]).all()) and bool(torch.isnan(r["loss"]))
    assert bool(torch.isnan(a["row_ws"][0, 2])) and int(torch.isnan(a["row_ws"]).sum()) == 1
    R.check_elem("sce label = V gradient", a["dl"][:, :V], r["grad"], r["b_grad"], alt=r["alt"])
    assert float(a["dl"][:, V:].abs().sum()) == 0.0


@TYPES
def test_sce_loss_refuses_a_row_wider_than_the_register_tile(ops, dtype):
    V = S["sce_refused"][dtype]
    v = R.vec_of(dtype)
    lg = torch.zeros(2, up(V, v), dtype=dtype, device=DEV)
    ids = torch.zeros(1, 3, dtype=torch.int64, device=DEV)
    loss, ws = torch.zeros(1, device=DEV), torch.zeros(6, device=DEV)
    for dl in (None, torch.zeros_like(lg)):
        with pytest.raises(ValueError, match="VCT_E_SHAPE"):
            ops.sce_loss(lg, V, ids[:, 1:], 2, -1, 1.0, loss, dl, ws)


def test_sce_measure_exp(ops, capsys):
    """The measured figure behind row_ref.SCE_EXP_REL: max |p_kernel - p| / p over the fp32 rows of this file at alpha = 1, where the
    gradient off the label is p / nvalid (valid rows; p >= 1e-30: above the fp32 denormals after the division).  The constant recorded
    in row_ref.py must still cover it with its factor of four, and must stay below the per-row figure of the older test."""
    worst = 0.0
    for V in S["sce_V"][F32]:
        x, ids, pad = R.sce_case(V, 40, F32)
        x, ids = x.to(DEV), ids.to(DEV)
        r = R.sce(x, ids[:, 1:].reshape(-1), 1.0, pad, F32)
        a = sce_run(ops, F32, V, 1.0, "separate", x, ids, pad)
        pk = a["dl"][:, :V].double() * r["nvalid"]
        sel = r["valid"][:, None] & (r["p"] >= 1e-30)
        sel[torch.arange(x.shape[0], device=DEV), r["y"]] = False
        if bool(sel.any()):
            worst = max(worst, float(((pk - r["p"]).abs() / r["p"])[sel].max()))
    capsys.readouterr()
    with capsys.disabled():
        print(f"\n[row] sce_loss: measured max |p_kernel - p| / p (__expf, the sum, the reciprocal) = {worst:.3e}; "
              f"recorded {R.SCE_EXP_REL:.3e}, allowed {R.SCE_EXP_ALLOW:.3e}")
    assert worst <= R.SCE_EXP_ALLOW <= R.SCE_CAP[F32]


# ---- embedding -------------------------------------------------------------------------------------------------------------------------------
def embed_bwd_run(ops, dtype, ids, Sq, V, pad, dx, dk, live0=None):
    N, d = dx.shape
    flat = ids[:, :Sq].reshape(-1)
    dead = (flat == pad) | (flat < 0) | (flat >= V)
    dxg = guard(dx)
    dxg[dead] = NAN                                     # rows no position owns: never read

    def build():
        a = Arena([mat("dtable", V, d, F32), ("id_ws", 1, 2 * V + 4 + N, torch.int32, 2 * V + 4 + N, 0), ("live", 1, V, torch.uint8, V, 0)])
        a["live"].zero_()
        ops.embed_bwd(ids[:, :Sq], Sq, pad, dxg, a["dtable"], dropout=dk, id_ws=a["id_ws"].view(-1), live=a["live"].view(-1))
        return a, None
    a, _ = twice(build)
    live = torch.zeros(V, dtype=torch.uint8, device=DEV)
    live[flat[~dead]] = 1
    assert torch.equal(a["live"].view(-1), live), "live rows"
    return a


@TYPES
def test_embed_fwd_bwd(ops, dtype, capsys):
    """vct_embed_fwd and vct_embed_bwd_live through the batch-stride view ids[:, :S]: tokens seen 1, 8, 9 and 40 times (the light /
    heavy split at 8 | 9), 1100 positions of one token (heavy), a light token whose scan takes a second trip, pads, an id equal to V
    and an id of -1 (no row, nothing written), d from one lane to the register limit, p in {0, 0.3}; integer dx at p = 0 bit-exact."""
    worst = 0.0
    for kind in S["emb_kinds"]:
        ids, Sq, V, pad = R.embed_ids(kind)
        ids = ids.to(DEV)
        flat = ids[:, :Sq].reshape(-1)
        N = flat.numel()
        for d in S["emb_d"]:
            if d % R.vec_of(dtype):
                continue
            for p in S["emb_p"]:
                dk, dr = drop_of(p)
                mask = R.drop_mask(N, d, dr, DEV) if dr else None
                tag = f"embed {kind} d={d} p={p}"
                dx = R.rnd((N, d), 71, 1.0, dtype, DEV)
                ref, e, _ = R.embed_bwd(flat, dx, V, pad, mask)
                a = embed_bwd_run(ops, dtype, ids, Sq, V, pad, dx, dk)
                worst = max(worst, R.check_elem(f"{tag} dtable", a["dtable"], ref, R.bound(ref, e, F32)))
                if p == 0.0:
                    dxi = R.G.ints((N, d), 70, dtype, DEV)
                    R.check_exact(f"{tag} dtable, integer dx", embed_bwd_run(ops, dtype, ids, Sq, V, pad, dxi, None)["dtable"],
                                  R.embed_bwd(flat, dxi, V, pad)[0])
                if kind != "mixed":
                    continue
                # forward (every id inside the table: the two outside become token 9); NaN in the table rows nobody reads
                good = torch.where((ids >= 0) & (ids < V), ids, torch.full_like(ids, 9))
                gflat = good[:, :Sq].reshape(-1)
                table = torch.full((V, d), NAN, device=DEV)
                used = torch.unique(gflat)
                table[used] = R.rnd((V, d), 60, 1.0, F32, DEV)[used]
                pos = guard(R.rnd((Sq, d), 61, 1.0, F32, DEV))

                def build():
                    b = Arena([mat("x", N, d, dtype)])
                    ops.embed_fwd(good[:, :Sq], Sq, table, pos, b["x"], dropout=dk)
                    return b, None
                b, _ = twice(build)
                x, ex = R.embed_fwd(gflat, torch.nan_to_num(table), pos, Sq, mask)
                bx = R.bound(x, ex, dtype)
                worst = max(worst, R.check_elem(f"{tag} x", b["x"], x, bx))
                if mask is not None:
                    R.check_mask(f"{tag} x mask", b["x"], x, bx)
    report(capsys, f"embed_fwd / embed_bwd {dtype}", worst)


@TYPES
def test_embed_bwd_exclusive_chain(ops, dtype):
    """exclusive on and off across two different batches on one table: the incremental call zeroes only the rows the call before it
    wrote, and the table must equal the second batch's gradient everywhere (integer dx: bit for bit)."""
    idsA, Sq, V, pad = R.embed_ids("mixed")
    idsB = torch.where(idsA >= 10, 10 + (idsA - 10 + 57) % 300, idsA)
    idsA, idsB = idsA.to(DEV), idsB.to(DEV)
    N, d = idsA.shape[0] * Sq, 64
    dxA, dxB = R.G.ints((N, d), 80, dtype, DEV), R.G.ints((N, d), 81, dtype, DEV)
    refA = R.embed_bwd(idsA[:, :Sq].reshape(-1), dxA, V, pad)[0]
    refB = R.embed_bwd(idsB[:, :Sq].reshape(-1), dxB, V, pad)[0]
    assert not torch.equal(refA != 0, refB != 0)

    def build():
        a = Arena([mat("dtable", V, d, F32)])
        t = a["dtable"]
        ops.embed_bwd(idsA[:, :Sq], Sq, pad, dxA, t)                     # not exclusive: a full zero-fill, and the chain is broken
        ops.embed_bwd(idsA[:, :Sq], Sq, pad, dxA, t, exclusive=True)      # first of a chain: still the full zero-fill
        first = t.clone()
        ops.embed_bwd(idsB[:, :Sq], Sq, pad, dxB, t, exclusive=True)      # incremental: only A's rows are zeroed
        second = t.clone()
        ops.embed_bwd(idsA[:, :Sq], Sq, pad, dxA, t)                     # exclusive off again
        return a, (first, second)
    a, (first, second) = twice(build)
    R.check_exact("exclusive chain, first call", first, refA)
    R.check_exact("exclusive chain, incremental call", second, refB)
    R.check_exact("exclusive off after the chain", a["dtable"], refA)


# ---- Adam -----------------------------------------------------------------------------------------------------------------------------------
HP = (1e-3, 0.9, 0.999, 1e-8)


def adam_run(ops, n, vals, step, wd, by_device, bump, skip):
    p, g, m, v = vals
    gg = guard(g)
    a = Arena([vec("p", n), vec("m", n), vec("v", n), vec("shadow", n, BF), ("step", 1, 1, torch.int32, 1, 0)])
    a["p"][0], a["m"][0], a["v"][0] = p, m, v
    a["step"].fill_(step)
    if by_device:
        hyper = torch.tensor([*HP, wd], dtype=F32, device=DEV)
        ops.adam_step(a["p"], gg, a["m"], a["v"], a["shadow"], 0.0, 0.0, 0.0, 0.0, 0.0, a["step"], skip=skip, bump=bump, hyper=hyper)
    else:
        ops.adam_step(a["p"], gg, a["m"], a["v"], a["shadow"], *HP, wd, a["step"], skip=skip, bump=bump)
    return a


def test_adam_step(ops, capsys):
    """vct_adam_step against torch.optim.Adam's formula in fp64: the bias corrections from the device counter (t = step + 1), the
    decay order, hyper-parameters by argument and by the device block (bit-identical), a shadow skip range inside the buffer, the bump.
    The sizes above a million elements (the last takes the grid-stride loop into its second trip) run one combination."""
    worst = 0.0
    for n in S["adam_n"]:
        vals = R.adam_case(n, 50, DEV)
        big = n > 4096
        for step in ((1,) if big else S["adam_step"]):
            for wd in ((0.01,) if big else S["adam_wd"]):
                r = R.adam(*vals, *HP, wd, step)
                skip = (8, 16) if n >= 1020 else (0, 0)
                runs = {}
                for by_device, bump in ((False, True), (True, False)):
                    a, _ = twice(lambda: (adam_run(ops, n, vals, step, wd, by_device, bump, skip), None), nonfinite_ok=("shadow",))
                    assert int(a["step"]) == step + (1 if bump else 0), "the step counter"
                    runs[by_device] = a
                    if big and by_device:
                        continue
                    tag = f"adam n={n} step={step} wd={wd} {'device block' if by_device else 'arguments'}"
                    worst = max(worst, R.check_elem(f"{tag} p", a["p"], r["p"][None], R.bound(r["p"], r["e_p"], F32)[None]),
                                R.check_elem(f"{tag} m", a["m"], r["m"][None], R.bound(r["m"], r["e_m"], F32)[None]),
                                R.check_elem(f"{tag} v", a["v"], r["v"][None], R.bound(r["v"], r["e_v"], F32)[None]))
                    keep = torch.ones(n, dtype=torch.bool, device=DEV)
                    keep[skip[0]:skip[1]] = False
                    sh = a["shadow"][0]
                    assert torch.equal(sh[keep], a["p"][0].to(BF)[keep]), f"{tag}: shadow != bf16(p)"
                    assert bool((sh[~keep].view(torch.int16) == -1).all()), f"{tag}: the skipped shadow range was written"
                    # the special elements: nothing but decay; v from 0; a gradient whose square is a denormal
                    decay = 1.0 - torch.tensor(HP[0], dtype=F32) * torch.tensor(wd, dtype=F32)
                    assert float(a["p"][0, 0]) == float(vals[0][0].cpu() * decay), f"{tag}: g = m = v = 0 must only decay"
                    assert float(a["m"][0, 0]) == 0.0 and float(a["v"][0, 0]) == 0.0 and float(a["v"][0, 1]) > 0.0
                for k, bits in (("p", torch.int32), ("m", torch.int32), ("v", torch.int32), ("shadow", torch.int16)):
                    assert torch.equal(runs[False][k].view(bits), runs[True][k].view(bits)), (n, step, wd, k, "device block differs from arguments")
    report(capsys, "adam_step", worst)
