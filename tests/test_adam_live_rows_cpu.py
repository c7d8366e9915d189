"""Host side of the optimizer's row-aware pass (no GPU): the fp32 argument that a never-used embedding row is a fixed point of the
update (tests/adam_live_ref.py restates csrc/vct_adam_core.h), the reference for the marks, the descriptor tables ops builds, and
the argument checks of the new entry points."""
import ctypes

import numpy as np
import pytest

import adam_live_ref as R


@pytest.mark.parametrize("t", [1, 2, 1000, 100000])
@pytest.mark.parametrize("lr,b1,b2,eps", [(1e-4, 0.9, 0.999, 1e-8), (1e-3, 0.0, 0.0, 1e-30), (0.5, 0.9999, 0.99999, 1.0), (0.0, 0.5, 0.5, 1e-8),
                                         (1e30, 0.9999, 0.99999, 1e-38)])
def test_a_zero_row_is_a_fixed_point_when_the_skip_condition_holds(lr, b1, b2, eps, t):
    """g = m = v = 0 under the kernel's condition, its corners included: p, m and v come back bit for bit, for any p (denormals,
    -0.0 and huge values too)."""
    assert R.zero_row_is_noop(lr, b1, b2, eps, 0.0, t)
    c = R.adam_consts(lr, b1, b2, eps, 0.0, t)
    assert c["decay"] == 1 and np.isfinite(c["step_size"]) and c["bc2s"] > 0
    rng = np.random.default_rng(t)
    p = np.concatenate([rng.standard_normal(4096).astype(np.float32), np.float32([0.0, -0.0, 1e-42, -1e-42, 3e38, -3e38, 1.0])])
    z = np.zeros_like(p)
    p2, m2, v2 = R.adam_update(p, z, z, z, c)
    assert np.array_equal(p2.view(np.uint32), p.view(np.uint32))
    assert not m2.view(np.uint32).any() and not v2.view(np.uint32).any()


def test_the_skip_condition_refuses_what_moves_a_zero_row():
    ok = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.0, t=3)
    assert R.zero_row_is_noop(**ok)
    assert not R.zero_row_is_noop(**{**ok, "wd": 0.01})              # every parameter decays
    assert not R.zero_row_is_noop(**{**ok, "eps": 0.0})              # 0 / 0
    assert not R.zero_row_is_noop(**{**ok, "eps": float("inf")})
    assert not R.zero_row_is_noop(**{**ok, "lr": float("inf")})      # inf * 0
    assert not R.zero_row_is_noop(**{**ok, "lr": float("nan")})
    assert not R.zero_row_is_noop(**{**ok, "lr": -1e-3})             # +0 + p turns p = -0.0 into +0.0
    assert not R.zero_row_is_noop(**{**ok, "b1": 1.0})               # bias correction 1 - 1^t = 0: infinite step size
    assert not R.zero_row_is_noop(**{**ok, "b2": 1.0})               # sqrt(0) / 0
    assert not R.zero_row_is_noop(**{**ok, "b1": -0.1}) and not R.zero_row_is_noop(**{**ok, "b2": float("nan")})
    # a decay that rounds to 1 in fp32 changes no parameter either: the condition is on 1 - lr * wd, not on wd
    assert R.zero_row_is_noop(**{**ok, "lr": 1e-6, "wd": 1e-3})
    # what the condition refuses really is no fixed point ...
    for bad in ({"wd": 0.01}, {"eps": 0.0}, {"lr": float("inf")}, {"b2": 1.0}):
        c = R.adam_consts(**{**ok, **bad})
        p2, m2, v2 = R.adam_update(np.float32(1), np.float32(0), np.float32(0), np.float32(0), c)
        assert p2.view(np.uint32) != 0x3f800000 or m2.view(np.uint32) != 0 or v2.view(np.uint32) != 0, bad
    # ... and -0.0 in a moment is none (m: -0 -> +0), which is why the rebuild looks at bits
    c = R.adam_consts(**ok)
    _, m2, _ = R.adam_update(np.float32(1), np.float32(0), np.float32(-0.0), np.float32(0), c)
    assert m2.view(np.uint32) == 0
    assert R.live_from_buffers(np.float32([[0, -0.0], [0, 0]]))[0] == 1


def test_marks_reference():
    ids = np.array([[101, 5, 0, 0], [101, 299, 300, -1], [7, 2 ** 31 + 7, 5, 0]], np.int64)
    live = R.marked_rows(ids, 0, 300)
    assert sorted(np.flatnonzero(live)) == [5, 7, 101, 299]


def test_range_tables_carry_the_row_descriptors():
    import torch
    from vct_amd import _lib, ops
    assert ctypes.sizeof(_lib.AdamRows) == 24 and _lib.AdamRows.live.offset == 16 and _lib.AdamRows.row_len.offset == 8
    live = torch.zeros(300, dtype=torch.uint8)
    ranges = [(0, 1000, True), (1024, 1024 + 300 * 96 + 64, False)]
    plain = ops.adam_ranges_table(ranges, "cpu")
    assert len(plain) == 3 and plain[1] == 2 and plain[2] == 1 + (300 * 96 + 64 + 4095) // 4096
    tab, n, blocks, rtab, keep = ops.adam_ranges_table(ranges, "cpu", {1: (1024, 96, 300, live)})
    assert (n, blocks) == plain[1:] and torch.equal(tab, plain[0]) and keep[0] is live
    rows = (_lib.AdamRows * 2).from_buffer_copy(rtab.numpy().tobytes())
    assert rows[0].live is None and rows[0].row_len == 0                      # the bias-like range: no table, stepped densely
    assert (rows[1].origin, rows[1].row_len, rows[1].nrows, rows[1].live) == (1024, 96, 300, live.data_ptr())
    with pytest.raises(AssertionError):
        ops.adam_ranges_table(ranges, "cpu", {0: (0, 4, 250, live)})          # a range with a shadow takes no row table
    with pytest.raises(AssertionError):
        ops.adam_ranges_table(ranges, "cpu", {1: (1024, 96, 301, live)})      # more rows than flags


def test_new_entry_points_refuse_bad_arguments_before_any_launch():
    import __graft_entry__ as g
    g.build()
    from vct_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 16)()
    p = ctypes.addressof(buf)
    assert lib.vct_embed_live_rebuild(4, 4, None, None, p, p, None) == -1
    assert lib.vct_embed_live_rebuild(4, 4, None, p, p, None, None) == -1
    assert lib.vct_embed_live_rebuild(0, 4, None, p, p, p, None) == -2
    assert lib.vct_adam_step_ranges_rows(p, p, p, p, None, None, 1, 1, 0, 0, 0, 0, 0, p, None, None, 0, p, None) == -1
    assert lib.vct_adam_step_ranges_rows(p, p, p, p, None, p, 1, 1, 0, 0, 0, 0, 0, p, None, None, 0, p + 4, None) == -3
    assert lib.vct_embed_bwd_live(_lib.BF16, 1, 1, 64, 8, None, 1, 0, p, p, p, 64, 0, None, 0, 0.0, p, None) == -1
