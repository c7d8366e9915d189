"""Fused Adam / AdamW over the flat parameter buffers (csrc/vct_optim.hip)."""
import torch

from .. import _lib as L


def adam_step(param, grad, exp_avg, exp_avg_sq, shadow, lr, beta1, beta2, eps, weight_decay, step_dev, skip=(0, 0), bump=True,
              hyper=None, pack=None):
    """Fused Adam/AdamW over flat fp32 buffers (+ bf16 shadow refresh).  step_dev: int32[1] device counter.
    `param` may be a slice of the flat buffer (range-by-range stepping): pass the same slice of every buffer,
    `skip` relative to the slice start, bump=False, and finish with adam_bump(step_dev).  hyper: device fp32 [5]
    (lr, beta1, beta2, eps, weight_decay) read by the kernel instead of the scalars (graph / launch-list replays)."""
    if pack is not None:      # (device table of vct_adam_pack_seg, entries, flat index of param[0]): packed weight copies written in the same pass
        table, nseg, base = pack
        L.check(L.load().vct_adam_step_pk(param.data_ptr(), grad.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(), L.ptr(shadow),
                                          param.numel(), float(lr), float(beta1), float(beta2), float(eps), float(weight_decay),
                                          step_dev.data_ptr(), int(skip[0]), int(skip[1]), int(bool(bump)), L.ptr(hyper),
                                          table.data_ptr(), int(nseg), int(base), L.stream_ptr()), "vct_adam_step_pk")
        return
    L.check(L.load().vct_adam_step(param.data_ptr(), grad.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(), L.ptr(shadow),
                                   param.numel(), float(lr), float(beta1), float(beta2), float(eps), float(weight_decay),
                                   step_dev.data_ptr(), int(skip[0]), int(skip[1]), int(bool(bump)), L.ptr(hyper), L.stream_ptr()),
            "vct_adam_step")


def adam_ranges_table(ranges, device, rows=None):
    """Device table for adam_step_ranges: ranges = sorted [(begin, end, has_shadow)] of flat elements (multiples of 4).
    Returns (table tensor, entries, workgroups).  rows = {range index: (origin, row_len, nrows, live uint8 tensor)}: those ranges lie
    inside a row-major table (row 0 at flat element `origin`) with a per-row live table, and the pass skips the rows that are not
    live (include/vct_hip.h, vct_adam_rows); the result then carries the device row table (and the live tensors) behind the three."""
    EPB = 4096
    arr = (L.AdamRange * len(ranges))()
    blk = 0
    for i, (a, b, sh) in enumerate(ranges):
        assert a % 4 == 0 and b % 4 == 0 and b > a
        arr[i].begin, arr[i].end, arr[i].blk0, arr[i].shadow = int(a), int(b), blk, int(bool(sh))
        blk += (b - a + EPB - 1) // EPB
    table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(device)
    if not rows:
        return table, len(ranges), blk
    rarr = (L.AdamRows * len(ranges))()
    for i, (origin, row_len, nrows, live) in rows.items():
        assert 0 <= i < len(ranges) and not ranges[i][2], "a range with a bf16 shadow is stepped densely: give it no row table"
        assert row_len > 0 and row_len % 4 == 0 and origin % 4 == 0 and live.dtype == torch.uint8 and live.numel() >= nrows
        rarr[i].origin, rarr[i].row_len, rarr[i].nrows, rarr[i].live = int(origin), int(row_len), int(nrows), live.data_ptr()
    rtable = torch.frombuffer(bytearray(bytes(rarr)), dtype=torch.uint8).to(device)
    return table, len(ranges), blk, rtable, [r[3] for r in rows.values()]


def adam_step_ranges(param, grad, exp_avg, exp_avg_sq, shadow, table, lr, beta1, beta2, eps, weight_decay, step_dev, hyper=None, pack=None):
    """vct_adam_step over a LIST of ranges of the WHOLE flat buffers in one launch (table from adam_ranges_table): what is left for a
    separate pass when the weight matrices are stepped inside their weight-gradient GEMMs.  pack = (device table of
    vct_adam_pack_seg with flat indices, entries) or None.  No step-counter bump.  A table built with rows skips the rows that are
    not live (same bits: a skipped row is one the update would not change)."""
    tab, n, blocks = table[:3]
    pk, nseg = (pack[0].data_ptr(), int(pack[1])) if pack is not None and pack[1] else (0, 0)
    if len(table) > 3:
        L.check(L.load().vct_adam_step_ranges_rows(param.data_ptr(), grad.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(),
                                                   L.ptr(shadow), tab.data_ptr(), int(n), int(blocks), float(lr), float(beta1),
                                                   float(beta2), float(eps), float(weight_decay), step_dev.data_ptr(), L.ptr(hyper), pk,
                                                   nseg, table[3].data_ptr(), L.stream_ptr()), "vct_adam_step_ranges_rows")
        return
    L.check(L.load().vct_adam_step_ranges(param.data_ptr(), grad.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(), L.ptr(shadow),
                                          tab.data_ptr(), int(n), int(blocks), float(lr), float(beta1), float(beta2), float(eps),
                                          float(weight_decay), step_dev.data_ptr(), L.ptr(hyper), pk, nseg, L.stream_ptr()),
            "vct_adam_step_ranges")


def adam_step_2d(param, grad, exp_avg, exp_avg_sq, shadow, shadow_t, lr, beta1, beta2, eps, weight_decay, step_dev, hyper=None):
    """vct_adam_step on one 2-D weight (views [rows, cols] of the flat buffers) that also writes the transposed bf16 shadow
    shadow_t [cols, ld >= rows] in the same pass."""
    rows, cols = param.shape
    L.check(L.load().vct_adam_step_2d(param.data_ptr(), grad.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(), L.ptr(shadow),
                                      shadow_t.data_ptr(), rows, cols, shadow_t.stride(0), float(lr), float(beta1), float(beta2),
                                      float(eps), float(weight_decay), step_dev.data_ptr(), L.ptr(hyper), L.stream_ptr()),
            "vct_adam_step_2d")


def adam_bump(step_dev):
    L.check(L.load().vct_adam_step(step_dev.data_ptr(), step_dev.data_ptr(), step_dev.data_ptr(), step_dev.data_ptr(), 0, 0,
                                   0.0, 0.0, 0.0, 0.0, 0.0, step_dev.data_ptr(), 0, 0, 1, 0, L.stream_ptr()), "vct_adam_step(bump)")
