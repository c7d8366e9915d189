"""Kernel-level tests (GPU) of vct_sce_loss_ls through vct_amd.ops.sce_loss_ls: loss, the (NLL, accuracy) pair, the per-row workspace
and every gradient element against the fp64 reference and the derived bounds of tests/label_smoothing_ref.py (itself checked by
tests/test_label_smoothing_cpu.py, which also shows that each checker used here rejects the fault meant for it).

Harness as in tests/test_row_kernels_gpu.py: outputs live in an Arena (0xFF everywhere, canaries around each), the logits carry NaN in
the columns V..ldl-1 and in the rows behind N -- a row sum that lost its mask turns the loss into NaN --, every call runs twice on
fresh arenas that must come out byte-identical.  Rows follow row_ref.sce_case (B 3, S 2): a dominant label column, a label below the
RCE clamp, a random row, a pad tail, an all-pad sequence.  The fp64 reference of a (V, alpha, eps) is computed once and shared by the
forms of the call."""
import pytest
import torch

import label_smoothing_ref as LS
import row_ref as R
from gpu_arena import Arena, up

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF = R.F32, R.BF
NAN = float("nan")
TYPES = pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
# vector tail; the switch between the two instantiations of a type; the width limit
SHAPES_V = {BF: (1, 7, 8, 9, 257, 32768, 32769, 65536), F32: (3, 4, 5, 16384, 16385, 32768)}
SWITCH = {BF: (257, 32769), F32: (257, 16385)}
LIMIT = {BF: 65536, F32: 32768}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from vct_amd import ops as _ops
    return _ops


def ls_run(ops, dtype, V, alpha, eps, form, x, ids, pad, ld_dl=None, legacy=False):
    """One form of the call on a fresh arena: 'separate' (ld_dl given or V rounded up), 'inplace' or 'forward'.  legacy: vct_sce_loss."""
    v = R.vec_of(dtype)
    N, vr = x.shape[0], up(V, v)
    labels = ids[:, 1:]
    nws = 2 * N + 1 if legacy else 4 * N + 1
    specs = [("loss", 1, 1, F32, 1, 0), ("stats", 1, 2, F32, 2, 0), ("row_ws", 1, nws, F32, nws + 1, 0)]
    if form == "inplace":
        a = Arena(specs + [("dl", N, vr, dtype, vr, 0)])
        a["dl"][:, :V] = x
        logits = dl = a["dl"]
    else:
        ldl = min(vr + v, LIMIT[dtype])
        buf = torch.full((N + 1, ldl), NAN, dtype=dtype, device=DEV)
        buf[:N, :V] = x
        logits = buf[:N]
        if form == "forward":
            a, dl = Arena(specs), None
        else:
            w = vr if ld_dl is None else ld_dl
            a = Arena(specs + [("dl", N, w, dtype, w, 0)])
            dl = a["dl"]
    if legacy:
        a["stats"].zero_()
        ops.sce_loss(logits, V, labels, labels.shape[1], pad, alpha, a["loss"], dl, a["row_ws"])
    else:
        ops.sce_loss_ls(logits, V, labels, labels.shape[1], pad, alpha, eps, a["loss"], dl, a["row_ws"], stats=a["stats"].view(-1))
    return a


def twice(build, nonfinite_ok=()):
    a1, a2 = build(), build()
    torch.cuda.synchronize()
    assert torch.equal(a1.buf, a2.buf), "two runs on fresh arenas differ"
    a1.check(nonfinite_ok)
    a2.check(nonfinite_ok)
    return a1


def ls_check(tag, a, r, alpha, N, grad=True):
    ws = a["row_ws"]
    w = [LS.check_loss(tag, a["loss"], r), LS.check_nll(tag, a["stats"], r), LS.check_acc(tag, a["stats"], r),
         LS.check_ce_rows(tag, ws[:, :N], r),
         R.check_elem(f"{tag} NLL rows", ws[:, 2 * N + 1:3 * N + 1], r["nll_rows"][None], r["b_nll"][None])]
    if alpha != 1.0:
        w.append(LS.check_rce_rows(tag, ws[:, N:2 * N], r))
    assert float(ws[0, 2 * N]) == r["nvalid"], "count of valid rows"
    R.check_exact(f"{tag} hit rows", ws[:, 3 * N + 1:4 * N + 1], r["hit_rows"].to(F32)[None])
    if grad:
        w.append(LS.check_grad(tag, a["dl"], r))
        LS.check_zeros(tag, a["dl"], r)
    return max(w)


@TYPES
def test_sce_loss_ls(ops, dtype, capsys):
    """Every V x eps x alpha, each in place, with a separate dlogits (ld_dl > V where the limit leaves room) and forward only."""
    worst, routes = 0.0, set()
    v = R.vec_of(dtype)
    for V in SHAPES_V[dtype]:
        x, ids, pad = R.sce_case(V, 40, dtype)
        x, ids = x.to(DEV), ids.to(DEV)
        N, vr = x.shape[0], up(V, v)
        wide = min(vr + v, LIMIT[dtype])
        for alpha in (1.0, 0.5):
            for eps in (0.1, 0.5):
                r = LS.sce_ls(x, ids[:, 1:].reshape(-1), alpha, eps, pad, dtype)
                got = {}
                for form in ("inplace", "separate", "forward"):
                    ld = wide if form == "separate" else None
                    a = twice(lambda: ls_run(ops, dtype, V, alpha, eps, form, x, ids, pad, ld))
                    worst = max(worst, ls_check(f"ls V={V} alpha={alpha} eps={eps} {form}", a, r, alpha, N, grad=form != "forward"))
                    routes.add(R.sce_tile(V, 0 if form == "forward" else (wide if form == "separate" else vr), dtype)[1])
                    got[form] = a
                # in place and forward only share an instantiation: the same loss, statistics and rows, bit for bit
                for name in ("loss", "stats", "row_ws"):
                    assert torch.equal(got["inplace"][name], got["forward"][name]), (V, alpha, eps, name)
    assert len(routes) == 2, routes
    capsys.readouterr()
    with capsys.disabled():
        print(f"\n[ls] sce_loss_ls {dtype}: instantiations reached {sorted(routes)}, worst |delta| / bound = {worst:.3f}")


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


@TYPES
@pytest.mark.parametrize("alpha", [1.0, 0.5])
def test_zero_smoothing_is_vct_sce_loss_bit_for_bit(ops, dtype, alpha):
    """Loss, gradient (signed zeros included), CE / RCE rows and count, in both instantiations of the type, in place and separate."""
    v = R.vec_of(dtype)
    for V in SWITCH[dtype]:
        x, ids, pad = R.sce_case(V, 44, dtype)
        x, ids = x.to(DEV), ids.to(DEV)
        N = x.shape[0]
        for form, ld in (("inplace", None), ("separate", up(V, v) + v), ("forward", None)):
            new = twice(lambda: ls_run(ops, dtype, V, alpha, 0.0, form, x, ids, pad, ld))
            old = twice(lambda: ls_run(ops, dtype, V, alpha, 0.0, form, x, ids, pad, ld, legacy=True))
            assert torch.equal(_bits(new["loss"]), _bits(old["loss"])), (V, form)
            assert torch.equal(_bits(new["row_ws"][:, :2 * N + 1]), _bits(old["row_ws"][:, :2 * N + 1])), (V, form)
            if form != "forward":
                assert torch.equal(_bits(new["dl"]), _bits(old["dl"])), (V, form)
            # at eps = 0 the NLL is the CE term
            assert float(new["stats"][0, 0]) == float(new["loss"]) or alpha != 1.0


@TYPES
def test_tie_with_the_label_on_the_later_column_is_a_hit(ops, dtype):
    V = 9
    x, ids, pad = LS.tie_case(V, dtype)
    x, ids = x.to(DEV), ids.to(DEV)
    r = LS.sce_ls(x, ids[:, 1:].reshape(-1), 1.0, 0.1, pad, dtype)
    assert float(r["stats"][1]) == 0.5
    a = twice(lambda: ls_run(ops, dtype, V, 1.0, 0.1, "separate", x, ids, pad))
    assert float(a["stats"][0, 1]) == 0.5
    ls_check("ls tie", a, r, 1.0, x.shape[0])


@TYPES
def test_label_outside_the_vocabulary(ops, dtype):
    """NaN loss and NaN NLL, the row counted as a miss, finite gradients against column 0, nothing written outside the outputs."""
    V, alpha, eps = 257, 0.5, 0.1
    x, ids, pad = R.sce_case(V, 42, dtype, oob=True)
    x, ids = x.to(DEV), ids.to(DEV)
    N = x.shape[0]
    r = LS.sce_ls(x, ids[:, 1:].reshape(-1), alpha, eps, pad, dtype)
    a = twice(lambda: ls_run(ops, dtype, V, alpha, eps, "separate", x, ids, pad), nonfinite_ok=("loss", "stats", "row_ws"))
    assert bool(torch.isnan(a["loss"]).all()) and bool(torch.isnan(r["loss"]))
    assert bool(torch.isnan(a["stats"][0, 0])) and not bool(torch.isnan(a["stats"][0, 1]))
    LS.check_acc("ls label = V", a["stats"], r)
    ws = a["row_ws"]
    assert bool(torch.isnan(ws[0, 2])) and bool(torch.isnan(ws[0, 2 * N + 1 + 2])) and int(torch.isnan(ws).sum()) == 2
    LS.check_grad("ls label = V", a["dl"], r)
    LS.check_zeros("ls label = V", a["dl"], r)


@TYPES
def test_all_pad_batch_behaves_as_vct_sce_loss(ops, dtype):
    V = 257
    x, ids, pad = R.sce_case(V, 45, dtype)
    ids[:, 1:] = pad
    x, ids = x.to(DEV), ids.to(DEV)
    for alpha in (1.0, 0.5):
        new = twice(lambda: ls_run(ops, dtype, V, alpha, 0.1, "separate", x, ids, pad), nonfinite_ok=("loss", "stats"))
        old = twice(lambda: ls_run(ops, dtype, V, alpha, 0.0, "separate", x, ids, pad, legacy=True), nonfinite_ok=("loss",))
        assert torch.equal(_bits(new["loss"]), _bits(old["loss"])) and torch.equal(_bits(new["dl"]), _bits(old["dl"]))
        assert bool(torch.isnan(new["stats"]).all())            # 0 / 0, as the loss's CE term


@TYPES
def test_refusals_return_their_codes_and_launch_nothing(ops, dtype):
    v = R.vec_of(dtype)
    V = 16 * v
    lg = torch.zeros(3, V + 1, dtype=dtype, device=DEV).view(-1)
    ids = torch.zeros(1, 3, dtype=torch.int64, device=DEV)
    aligned = lg[:2 * V].view(2, V)
    out = torch.full((64,), NAN, device=DEV)
    loss, stats, ws = out[0:1], out[4:6], out[8:8 + 10]

    def call(logits=aligned, Vc=V, eps=0.1, dl=None):
        ops.sce_loss_ls(logits, Vc, ids[:, 1:], 2, -1, 1.0, eps, loss, dl, ws, stats=stats)
    for eps in (1.0, -0.5, NAN, float("inf")):
        with pytest.raises(ValueError, match="VCT_E_ARG"):
            call(eps=eps)
    with pytest.raises(ValueError, match="VCT_E_ALIGN"):
        call(logits=lg[1:1 + 2 * V].view(2, V))                    # a base that is not 16-byte aligned
    with pytest.raises(ValueError, match="VCT_E_ALIGN"):
        call(dl=lg[1:1 + 2 * V].view(2, V))
    with pytest.raises(ValueError, match="VCT_E_ALIGN"):
        call(logits=torch.zeros(2, V + v, dtype=dtype, device=DEV)[:, :V + 1], Vc=V + 1 + v)     # ldl below V rounded up
    wide = LIMIT[dtype] + v
    big = torch.zeros(2, wide, dtype=dtype, device=DEV)
    for dl in (None, torch.zeros_like(big)):
        with pytest.raises(ValueError, match="VCT_E_SHAPE"):
            call(logits=big, Vc=wide, dl=dl)
    with pytest.raises(ValueError, match="VCT_E_SHAPE"):
        call(dl=big)                                                 # the gradient's row alone is too wide
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()), "a refused call wrote an output"
