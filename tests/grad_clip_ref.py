"""numpy fp64 definition of gradient clipping over explicit segments of a flat fp32 buffer: what torch.nn.utils.clip_grad_norm_ /
clip_grad_value_ compute on the tensors the segments stand for.  The checker of tests/test_grad_clip_*.py; nothing here is
imported by the package."""
import numpy as np

F32 = np.float32


def seg_sqsums(g, segments):
    """fp64 sum of squares of every segment (each fp32 product is exact in fp64)."""
    g = np.asarray(g)
    return [float(np.sum(np.square(g[a:b].astype(np.float64)))) for a, b in segments]


def norms(g, segments):
    """(norm fp32, seg_norm fp32 [n], total fp64 sum of squares): sqrt in fp64, then one rounding to fp32."""
    with np.errstate(over="ignore", invalid="ignore"):
        sq = seg_sqsums(g, segments)
        tot = 0.0
        for s in sq:                                         # ascending segment order
            tot += s
        return F32(np.sqrt(np.float64(tot))), np.sqrt(np.asarray(sq, np.float64)).astype(F32), tot


def coef_of(norm, max_norm):
    """torch: clip_coef = max_norm / (total_norm + 1e-6); clamp(clip_coef, max = 1.0) -- every operation in fp32; a NaN stays."""
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        q = F32(max_norm) / (F32(norm) + F32(1e-6))
    return F32(1.0) if q > F32(1.0) else F32(q)


def clip_by_norm(g, segments, max_norm):
    """(clipped copy of g, norm, coef, seg_norm): the segments times coef in fp32 (untouched when coef is exactly 1), everything
    outside the segments as it was."""
    g = np.asarray(g, F32)
    norm, seg_norm, _ = norms(g, segments)
    c = coef_of(norm, max_norm)
    out = g.copy()
    if not c == F32(1.0):
        with np.errstate(over="ignore", invalid="ignore"):
            for a, b in segments:
                out[a:b] = g[a:b] * c
    return out, norm, c, seg_norm


def clip_by_value(g, segments, v):
    """torch.clamp(g, -v, v) on the segments: NaN stays NaN, +-inf -> +-v, -0.0 stays -0.0."""
    g = np.asarray(g, F32)
    out = g.copy()
    v = F32(v)
    for a, b in segments:
        x = g[a:b]
        out[a:b] = np.where(x < -v, -v, np.where(x > v, v, x))
    return out


def ulps(a, b):
    """Distance of two fp32 numbers in units in the last place of fp32 (same sign, finite)."""
    ia = np.asarray(a, F32).view(np.int32).astype(np.int64)
    ib = np.asarray(b, F32).view(np.int32).astype(np.int64)
    return np.abs(ia - ib)


def same_bits(a, b):
    return np.array_equal(np.asarray(a, F32).view(np.uint32), np.asarray(b, F32).view(np.uint32))


def check(g_before, g_after, segments, norm, coef, seg_norm, max_norm, norm_ulps=1):
    """The acceptance check the GPU tests apply to a device result: norm and every seg_norm within norm_ulps of the fp64
    definition (NaN / inf: as the definition gives them), coef the fp32 formula on the DEVICE's norm bit for bit, every segment
    element fp32(g * coef) bit for bit, everything outside the segments untouched.  Returns a list of complaints (empty: pass)."""
    bad = []
    ref_norm, ref_seg, _ = norms(g_before, segments)

    def close(x, r, what):
        x, r = F32(x), F32(r)
        if np.isnan(r) or np.isinf(r):
            if not same_bits(x, r) and not (np.isnan(x) and np.isnan(r)):
                bad.append(f"{what}: {x} where the definition gives {r}")
        elif not np.isfinite(x) or ulps(x, r) > norm_ulps:
            bad.append(f"{what}: {x!r} vs {r!r}")
    close(norm, ref_norm, "norm")
    seg_norm = np.asarray(seg_norm, F32)
    if seg_norm.shape != ref_seg.shape:
        bad.append(f"seg_norm has {seg_norm.shape} entries for {len(segments)} segments")
    else:
        for i in range(len(segments)):
            close(seg_norm[i], ref_seg[i], f"seg_norm[{i}]")
    c = coef_of(norm, max_norm)
    if not (same_bits(coef, c) or (np.isnan(c) and np.isnan(F32(coef)))):
        bad.append(f"coef {coef!r} is not the fp32 formula on the returned norm ({c!r})")
    want = np.asarray(g_before, F32).copy()
    if not F32(coef) == F32(1.0):
        with np.errstate(over="ignore", invalid="ignore"):
            for a, b in segments:
                want[a:b] = want[a:b] * F32(coef)
    got = np.asarray(g_after, F32)
    inside = np.zeros(want.shape, bool)
    for a, b in segments:
        inside[a:b] = True
    # bits; inside a segment a NaN may come back with another payload, outside nothing may change at all
    diff = (want.view(np.uint32) != got.view(np.uint32)) & ~(inside & np.isnan(want) & np.isnan(got))
    if diff.any():
        i = int(np.flatnonzero(diff)[0])
        bad.append(f"element {i} ({'inside a segment' if inside[i] else 'OUTSIDE every segment'}): {got[i]!r}, expected {want[i]!r} "
                   f"({int(diff.sum())} differ)")
    return bad
