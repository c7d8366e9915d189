"""vct_ensemble_combine (csrc/vct_ensemble.hip) through ops.ensemble_combine against the fp64 reference and the per-element bound of
tests/ensemble_ref.py.  The output lives in a tests/gpu_arena.py arena (canaries on both sides, NaN in the padding columns, which
must stay untouched), every member's columns >= V hold NaN (a kernel that read them would write NaN), members mix fp32 and bf16,
row strides that keep and that break 16-byte row alignment, and a base that is not 16-byte aligned."""
import pytest
import torch

import ensemble_ref as ER
from gpu_arena import Arena, up

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF = ER.F32, ER.BF
VS = (1, 7, 8, 9, 255, 256, 257, 2051, 30522)
ROWS = (1, 2, 129)
MS = (1, 2, 3, 8)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _w_dev(w):
    return torch.tensor(list(w) + [0.0] * (8 - len(w)), dtype=torch.float32, device=DEV)


def _place(x, kind):
    """x [rows, V] on the device inside a NaN-filled buffer: kind 0 a row stride of up(V, 8) (rows 16-byte aligned), 1 that + 8
    (ld > V, still aligned), 2 a stride of V + 1 from a base one element into the buffer (neither base nor rows aligned)."""
    rows, V = x.shape
    ld, skew = ((up(V, 8), 0), (up(V, 8) + 8, 0), (V + 1, 1))[kind]
    raw = torch.full((rows * ld + skew,), float("nan"), dtype=x.dtype, device=DEV)
    view = raw[skew:].view(rows, ld)[:, :V]
    view.copy_(x)
    return view


def _run(xs, w, mode, rows, V, out_kind, place=None):
    """(out view, arena) of one call; member m is placed by kind (m + place) % 3."""
    from vct_amd import ops
    ld_out, skew = ((up(V, 4), 0), (up(V, 4) + 4, 0), (V + 1, 1))[out_kind]
    arena = Arena([("out", rows, V, F32, ld_out, skew)])
    views = [_place(x.to(DEV), (m + (place or 0)) % 3) for m, x in enumerate(xs)]
    ops.ensemble_combine(views, _w_dev(w), arena["out"], mode, cols=V)
    torch.cuda.synchronize()
    return arena["out"], arena, views


@pytest.mark.parametrize("mode", ER.MODES)
@pytest.mark.parametrize("V", VS)
def test_combine_within_the_bound(V, mode):
    case = 0
    for rows in ROWS:
        for n in MS:
            xs = ER.members(rows, V, n, seed=1000 * V + 10 * rows + n)
            if n == 1 and rows == 2:
                xs = [xs[0].to(BF)]                                     # (a lone bf16 member)
            w = ER.weights(n, seed=V + n)
            out, arena, _ = _run(xs, w, mode, rows, V, out_kind=case % 3, place=case)
            ref, bound = ER.combine([x.to(DEV) for x in xs], w, mode)
            ER.check(f"V {V} rows {rows} members {n} {mode}", out, ref, bound)
            arena.check()
            case += 1


@pytest.mark.parametrize("mode", ER.MODES)
def test_zero_weight_member_is_not_read(mode):
    rows, V = 3, 257
    xs = ER.members(rows, V, 3, seed=4)
    xs[1] = torch.full_like(xs[1], float("nan"))
    xs[1][:, 3] = float("-inf")
    w = [0.625, 0.0, 0.375]
    out, arena, _ = _run(xs, w, mode, rows, V, out_kind=0)
    ref, bound = ER.combine([xs[0].to(DEV), xs[2].to(DEV)], [0.625, 0.375], mode)
    ER.check(f"zero weight {mode}", out, ref, bound)
    arena.check()
    # ... and the weights are the device's: the same launch arguments with another block give the other pair
    from vct_amd import ops
    wd = _w_dev([0.0, 0.0, 1.0])
    views = [x.to(DEV) for x in xs]
    got = torch.empty(rows, V, dtype=F32, device=DEV)
    ops.ensemble_combine(views, wd, got, mode)
    ref, bound = ER.combine([views[2]], [1.0], mode)
    ER.check(f"weights (0, 0, 1) {mode}", got, ref, bound)


@pytest.mark.parametrize("dtypes", [(F32,), (BF, F32)], ids=["fp32", "bf16+fp32"])
def test_shift_by_the_largest_log_probability(dtypes):
    rows, V = 2, 257
    x0, x1 = ER.shift_case(rows, V, seed=9, dtypes=dtypes)
    for mode in ER.MODES:
        out, arena, _ = _run([x0, x1], [0.5, 0.5], mode, rows, V, out_kind=1)
        ref, bound = ER.combine([x0.to(DEV), x1.to(DEV)], [0.5, 0.5], mode)
        assert bool(torch.isfinite(ref[:, :3]).all()) and float(ref[:, 2].max()) < -150.0 and bool((ref[:, 3] == float("-inf")).all())
        ER.check(f"+80 / -80 {mode}", out, ref, bound)
        arena.check(nonfinite_ok=("out",))


@pytest.mark.parametrize("mode", ER.MODES)
def test_nan_stays_in_its_row(mode):
    rows, V = 3, 2051
    xs = ER.members(rows, V, 3, seed=6)
    xs[2][1, 1030] = float("nan")
    w = ER.weights(3, seed=1)
    out, arena, _ = _run(xs, w, mode, rows, V, out_kind=2)
    ref, bound = ER.combine([x.to(DEV) for x in xs], w, mode)
    assert bool(torch.isnan(ref[1]).all()) and bool(torch.isfinite(ref[[0, 2]]).all())
    ER.check(f"NaN row {mode}", out, ref, bound)
    arena.check(nonfinite_ok=("out",))


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("V", [9, 2051, 30522])
def test_exact_identities(V):
    from vct_amd import ops
    rows = 3
    for dtype in (F32, BF):
        x = ER.members(rows, V, 1, seed=V, dtypes=(dtype,))[0].to(DEV)
        one = torch.empty(rows, V, dtype=F32, device=DEV)
        two = torch.empty_like(one)
        ops.ensemble_combine([x], _w_dev([1.0]), one, "logp")
        ops.ensemble_combine([x, x], _w_dev([0.5, 0.5]), two, "logp")
        assert torch.equal(_bits(one), _bits(two)), "logp with weights (1/2, 1/2) on one tensor twice is the single member"
        ER.check("single member", one, *ER.combine([x], [1.0], "logp"))
    xs = [m.to(DEV) for m in ER.members(rows, V, 3, seed=V + 1)]
    wd = _w_dev(ER.weights(3, seed=2))
    for mode in ER.MODES:
        a, b = torch.empty(rows, V, dtype=F32, device=DEV), torch.empty(rows, V, dtype=F32, device=DEV)
        ops.ensemble_combine(xs, wd, a, mode)
        ops.ensemble_combine(xs, wd, b, mode)
        assert torch.equal(_bits(a), _bits(b)), "a second call gives the same bits"


def test_refusals_raise():
    from vct_amd import ops
    x = torch.zeros(4, 80, device=DEV)
    out = torch.full((4, 80), 7.0, device=DEV)
    w = _w_dev([1.0])
    with pytest.raises(ValueError):
        ops.ensemble_combine([], w, out)
    with pytest.raises(ValueError):
        ops.ensemble_combine([x] * 9, w, out)
    with pytest.raises(ValueError, match="VCT_E_SHAPE"):
        ops.ensemble_combine([x[:, :70]], w, out, cols=90)                   # ld_out >= V, but a member's ld < V ... (80 < 90)
    with pytest.raises(ValueError, match="VCT_E_SHAPE"):
        ops.ensemble_combine([x], w, out[:, :70].contiguous(), cols=80)      # ld_out < V
    with pytest.raises(KeyError):
        ops.ensemble_combine([x], w, out, mode="mean")
    with pytest.raises(TypeError):
        ops.ensemble_combine([x.half()], w, out)
    with pytest.raises(TypeError):
        ops.ensemble_combine([x], w.double(), out)
    with pytest.raises(ValueError):
        ops.ensemble_combine([x[:3]], w, out)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
