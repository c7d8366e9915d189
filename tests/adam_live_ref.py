"""CPU reference for the optimizer's row-aware pass over the token-embedding table (tests/test_adam_live_rows_*.py):
what the live table must hold, when a row may be skipped, and the update itself in fp32 (numpy)."""
import numpy as np

F = np.float32


def _fma(a, b, c):
    # float32 products are exact in float64; one more rounding to float32 (double rounding can differ from a true fma in the
    # last bit for general values -- exact for the zero rows this reference is about)
    return F(np.float64(a) * np.float64(b) + np.float64(c))


def adam_consts(lr, b1, b2, eps, wd, t):
    """csrc/vct_adam_core.h, adam_consts: t = steps already taken + 1."""
    lr, b1, b2, eps, wd = (F(x) for x in (lr, b1, b2, eps, wd))
    with np.errstate(all="ignore"):
        bc1 = F(1) - F(np.power(b1, F(t)))
        return dict(b1=b1, b2=b2, eps=eps, bc2s=F(np.sqrt(F(1) - F(np.power(b2, F(t))))), step_size=F(lr / bc1),
                    decay=F(F(1) - F(lr * wd)))


def adam_update(p, g, m, v, c):
    """csrc/vct_adam_core.h, adam_update, on float32 arrays; returns (p, m, v)."""
    p, g, m, v = (np.asarray(x, F) for x in (p, g, m, v))
    with np.errstate(all="ignore"):
        w0 = F(p * c["decay"])
        m2 = _fma(F(F(1) - c["b1"]), F(g - m), m)
        v2 = _fma(F(F(F(1) - c["b2"]) * g), g, F(c["b2"] * v))
        denom = F(F(np.sqrt(v2)) / c["bc2s"]) + c["eps"]
        p2 = _fma(-c["step_size"], F(m2 / denom), w0)
    return p2.astype(F), m2.astype(F), v2.astype(F)


def zero_row_is_noop(lr, b1, b2, eps, wd, t):
    """The kernel's skip condition (csrc/vct_optim.hip, adam_zero_row_is_noop): decay == 1, eps > 0 and a finite step size, in the
    form that needs no powf -- 0 <= b1 <= 0.9999, 0 <= b2 <= 0.99999, 0 <= lr <= 1e30, t >= 1."""
    lr, b1, b2, eps, wd = (F(x) for x in (lr, b1, b2, eps, wd))
    with np.errstate(all="ignore"):
        decay_is_one = F(F(1) - F(lr * wd)) == F(1) and F(np.float64(1) - np.float64(lr) * np.float64(wd)) == F(1)
    return bool(decay_is_one and eps > 0 and np.isfinite(eps) and 0 <= lr <= F(1e30) and 0 <= b1 <= F(0.9999)
                and 0 <= b2 <= F(0.99999) and t >= 1)


def marked_rows(ids, pad_id, V):
    """uint8 [V]: the rows a batch gives a gradient to -- every id inside [0, V) that is not the pad id."""
    ids = np.asarray(ids).reshape(-1)
    ok = (ids >= 0) & (ids < V) & (ids != pad_id)
    live = np.zeros(V, np.uint8)
    live[ids[ok]] = 1
    return live


def live_from_buffers(*tables):
    """uint8 [V]: rows with any BIT set in any of the fp32 [V, d] tables (-0.0 counts: it is not a fixed point of the update)."""
    any_ = np.zeros(tables[0].shape[0], bool)
    for t in tables:
        any_ |= (np.ascontiguousarray(t, F).view(np.uint32) != 0).any(axis=1)
    return any_.astype(np.uint8)
