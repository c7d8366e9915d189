"""Gradient clipping without a GPU: the numpy definition (tests/grad_clip_ref.py) against torch.nn.utils, the checker's power to
reject, the entry points' argument codes, the segment table's refusals and the settings' way through the optimizer."""
import ctypes
import math

import numpy as np
import pytest
import torch

import grad_clip_ref as R
import vct_oracle as O
from helpers import build_model, golden_params, load_golden, model_config_of

F32 = np.float32


def _tensors(seed, shapes, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(*s, generator=g) * scale for s in shapes]


def _flat(tensors, align=64):
    """The tensors laid out like the model's flat buffer (each at a multiple of `align`), NaN in the gaps: (flat, segments)."""
    segs, off = [], 0
    for t in tensors:
        segs.append((off, off + t.numel()))
        off += (t.numel() + align - 1) // align * align
    flat = np.full(off, np.nan, F32)
    for t, (a, b) in zip(tensors, segs):
        flat[a:b] = t.reshape(-1).numpy()
    return flat, segs


SHAPES = [(7,), (33, 5), (4101,), (1,), (64, 64)]


@pytest.mark.parametrize("scale,max_norm", [(1.0, 0.5), (1.0, 1e9), (1e-3, 1.0), (30.0, 2.0), (1.0, float("inf"))])
def test_reference_equals_torch_clip_grad_norm(scale, max_norm):
    ts = _tensors(1, SHAPES, scale)
    flat, segs = _flat(ts)
    out, norm, coef, seg_norm = R.clip_by_norm(flat, segs, max_norm)
    ps = [torch.nn.Parameter(torch.zeros_like(t)) for t in ts]
    for p, t in zip(ps, ts):
        p.grad = t.clone()
    total = torch.nn.utils.clip_grad_norm_(ps, max_norm)
    # torch accumulates the norm in fp32 (per tensor, then over the tensors): fp32 rounding of a few thousand terms away from the fp64
    # definition, 2e-6 relative at the most; the coefficient follows the norm
    assert abs(float(total) - float(norm)) <= 2e-6 * float(norm)
    t_coef = min(1.0, float(F32(max_norm) / (F32(float(total)) + F32(1e-6))))
    assert abs(t_coef - float(coef)) <= 4e-6 * float(coef)
    for p, t, (a, b), sn in zip(ps, ts, segs, seg_norm):
        assert abs(float(t.double().norm()) - float(sn)) <= np.spacing(sn)
        want = p.grad.reshape(-1).numpy()
        assert np.allclose(out[a:b], want, rtol=4e-6, atol=0.0)
        # and with torch's own coefficient the values are fp32 roundings of the same product
        assert np.array_equal(t.reshape(-1).numpy() * F32(coef), out[a:b]) or float(coef) == 1.0
    inside = np.zeros(flat.size, bool)
    for a, b in segs:
        inside[a:b] = True
    assert np.isnan(out[~inside]).all()                       # the gaps are no part of anything
    if max_norm in (1e9, float("inf")):
        assert coef == F32(1.0) and R.same_bits(out[inside], flat[inside])


def test_reference_equals_torch_clip_grad_value():
    ts = _tensors(2, SHAPES)
    ts[0][:4] = torch.tensor([float("nan"), float("inf"), -float("inf"), -0.0])
    flat, segs = _flat(ts)
    out = R.clip_by_value(flat, segs, 0.25)
    ps = [torch.nn.Parameter(torch.zeros_like(t)) for t in ts]
    for p, t in zip(ps, ts):
        p.grad = t.clone()
    torch.nn.utils.clip_grad_value_(ps, 0.25)
    for p, (a, b) in zip(ps, segs):
        want = p.grad.reshape(-1).numpy()
        assert np.array_equal(np.isnan(out[a:b]), np.isnan(want))
        ok = ~np.isnan(want)
        assert R.same_bits(out[a:b][ok], want[ok])
    assert np.isnan(out[0]) and out[1] == F32(0.25) and out[2] == F32(-0.25) and np.signbit(out[3]) and out[3] == 0.0


def test_reference_special_values():
    segs = [(0, 4)]
    assert R.norms(np.array([3e19, 3e19, 0, 0], F32), segs)[0] == F32(np.sqrt(2.0) * np.float64(F32(3e19)))
    assert R.norms(np.array([1e-30, 0, 0, 0], F32), segs)[0] == F32(1e-30)
    assert R.norms(np.zeros(4, F32), segs)[0] == 0.0 and R.coef_of(F32(0.0), 1.0) == F32(1.0)
    assert np.isnan(R.coef_of(F32(np.nan), 1.0))              # torch.clamp propagates NaN
    assert R.coef_of(F32(np.inf), 1.0) == F32(0.0)
    assert R.coef_of(F32(5.0), float("inf")) == F32(1.0)


def test_checker_rejects_wrong_results():
    ts = _tensors(3, [(7,), (4101,), (12,)])
    flat, segs = _flat(ts)
    out, norm, coef, seg_norm = R.clip_by_norm(flat, segs, 0.5)
    assert coef < 1 and R.check(flat, out, segs, norm, coef, seg_norm, 0.5) == []
    # a dropped segment: its squares are missing from the norm
    n2, _, _ = R.norms(flat, segs[:2])
    assert any("norm" in b for b in R.check(flat, out, segs, n2, R.coef_of(n2, 0.5), seg_norm, 0.5))
    # ... or it was not scaled
    o2 = out.copy(); o2[segs[2][0]:segs[2][1]] = flat[segs[2][0]:segs[2][1]]
    assert any("inside a segment" in b for b in R.check(flat, o2, segs, norm, coef, seg_norm, 0.5))
    # a padding element counted in (the padding holds a finite value here)
    f3 = flat.copy(); f3[7] = 100.0
    n3 = F32(np.sqrt(R.norms(f3, segs)[2] + 100.0 ** 2))
    assert any("norm" in b for b in R.check(f3, R.clip_by_norm(f3, segs, 0.5)[0], segs, n3, R.coef_of(n3, 0.5), seg_norm, 0.5))
    # a padding element written
    o4 = out.copy(); o4[8] = 0.0
    assert any("OUTSIDE" in b for b in R.check(flat, o4, segs, norm, coef, seg_norm, 0.5))
    # a coefficient applied when it should be 1
    out1, norm1, coef1, sn1 = R.clip_by_norm(flat, segs, 1e9)
    assert coef1 == F32(1.0)
    assert any("coef" in b for b in R.check(flat, out, segs, norm1, coef, sn1, 1e9))
    assert any("element" in b for b in R.check(flat, out, segs, norm1, coef1, sn1, 1e9))
    # one per-segment norm off by two ulps
    sn5 = seg_norm.copy(); sn5[1] = np.nextafter(np.nextafter(sn5[1], F32(np.inf)), F32(np.inf))
    assert any("seg_norm[1]" in b for b in R.check(flat, out, segs, norm, coef, sn5, 0.5))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from vct_amd import _lib
    return _lib.load()


def test_entry_points_return_codes_before_any_launch(lib):
    ARG, SHAPE, ALIGN = -1, -2, -3
    raw = (ctypes.c_char * 256)()
    p = (ctypes.addressof(raw) + 15) & ~15

    def sq(grad=p, segs=p, nseg=1, blocks=1, partials=p, seg_norm=p, clip=p, state=p):
        return lib.vct_grad_sqnorm(grad, segs, nseg, blocks, partials, seg_norm, clip, state, None)

    def ap(grad=p, segs=p, nseg=1, blocks=1, mode=0, clip=p, state=p):
        return lib.vct_grad_clip_apply(grad, segs, nseg, blocks, mode, clip, state, None)
    # every call below also carries a refusal: none may launch (there is no device here)
    for k in ("grad", "segs", "partials", "seg_norm", "clip", "state"):
        assert sq(**{k: None}, nseg=0) == ARG, k
    assert sq(nseg=0, grad=p + 4) == SHAPE and sq(nseg=-3, grad=p + 4) == SHAPE and sq(blocks=0, grad=p + 4) == SHAPE
    assert sq(grad=p + 4) == ALIGN and sq(grad=p + 8) == ALIGN and sq(partials=p + 8) == ALIGN and sq(segs=p + 8) == ALIGN
    for k in ("grad", "segs", "clip"):
        assert ap(**{k: None}, nseg=0) == ARG, k
    assert ap(state=None, nseg=0) == ARG                      # the norm mode reads the coefficient ...
    assert ap(state=None, mode=1, nseg=0) == SHAPE            # ... the value mode does not
    assert ap(mode=2, nseg=0) == ARG and ap(mode=-1, nseg=0) == ARG
    assert ap(nseg=0, grad=p + 4) == SHAPE and ap(blocks=-1, grad=p + 4) == SHAPE
    assert ap(grad=p + 4) == ALIGN and ap(segs=p + 8) == ALIGN and ap(grad=p + 8, mode=1) == ALIGN


def test_segment_table_layout_and_refusals():
    from vct_amd import _lib, ops
    tab, n, blocks = ops.grad_segments_table([(0, 7), (64, 64 + 4101), (8256, 8256 + 12)], "cpu")
    assert (n, blocks) == (3, 1 + 2 + 1) and tab.numel() == 3 * ctypes.sizeof(_lib.GradSeg)
    arr = (_lib.GradSeg * 3).from_buffer_copy(bytes(tab.numpy()))
    assert [(s.begin, s.end, s.blk0) for s in arr] == [(0, 7, 0), (64, 4165, 1), (8256, 8268, 3)]
    assert ops.grad_segments_table([(0, 4096), (4096, 8193)], "cpu")[2] == 3          # touching segments are disjoint
    for bad, what in (([(64, 80), (0, 7)], "sorted"), ([(0, 70), (64, 80)], "overlaps"), ([(2, 9)], "multiple of 4"),
                      ([(0, 8), (10, 12)], "multiple of 4"), ([(8, 8)], "empty"), ([], "no segments")):
        with pytest.raises(ValueError, match=what):
            ops.grad_segments_table(bad, "cpu")
    assert ops.grad_sqnorm_scratch((tab, n, blocks), "cpu").shape == (blocks + n,)


# ---- the settings -------------------------------------------------------------------------------------------------------------------
def _cpu_model():
    z = load_golden("tiny_train.npz")
    mc = model_config_of(z)
    cfg = O.cfg_from_model_config(mc, int(z["vocab"]))
    return build_model(mc, int(z["vocab"]), "cpu", torch.float32, golden_params(z, cfg))


TC = {"optimizer": {"name": "adam", "learning_rate": 1e-3, "beta": [0.9, 0.999], "weight_decay": 0}}


def _tc(**kw):
    return {"optimizer": dict(TC["optimizer"], **kw)}


def test_settings_live_in_the_param_group_and_survive_state_dict(tmp_path):
    from vct_amd import checkpoint as ck
    from vct_amd.trainer import FusedAdam, build_optimizer
    m = _cpu_model()
    plain = FusedAdam(m, lr=1e-3)
    assert "max_grad_norm" not in plain.param_groups[0] and "clip_grad_value" not in plain.param_groups[0]
    opt = FusedAdam(m, lr=1e-3, max_grad_norm=2.5)
    assert opt.param_groups[0]["max_grad_norm"] == 2.5 and "clip_grad_value" not in opt.param_groups[0]
    sd = opt.state_dict()
    assert sd["param_groups"][0]["max_grad_norm"] == 2.5
    plain.load_state_dict(sd)
    assert plain.param_groups[0]["max_grad_norm"] == 2.5
    assert FusedAdam(m, clip_grad_value=0.1).param_groups[0]["clip_grad_value"] == pytest.approx(0.1)
    assert FusedAdam(m, max_grad_norm=float("inf")).param_groups[0]["max_grad_norm"] == math.inf
    # the factory: every optimizer kind (a CPU model gets torch's Adam / AdamW / SGD)
    for tc in (_tc(max_grad_norm=1.5), _tc(max_grad_norm=1.5, weight_decay=0.01), {"optimizer": {"name": "sgd", "learning_rate": 0.1,
                                                                                              "momentum": 0.9, "max_grad_norm": 1.5}}):
        o, _ = build_optimizer(tc, m)
        assert o.param_groups[0]["max_grad_norm"] == 1.5
        o2, _ = build_optimizer(_tc() if tc["optimizer"]["name"] == "adam" else {"optimizer": {"name": "sgd", "learning_rate": 0.1, "momentum": 0.9}}, m)
        assert "max_grad_norm" not in o2.param_groups[0]
    o, _ = build_optimizer(_tc(clip_grad_value=0.5), m)
    assert o.param_groups[0]["clip_grad_value"] == 0.5
    # ... and through a training-state file
    path = str(tmp_path / "s.pt")
    ck.save_training_state(path, m, o, None, epoch=0)
    o3, _ = build_optimizer(_tc(), m)
    ck.load_training_state(path, m, o3)
    assert o3.param_groups[0]["clip_grad_value"] == 0.5


@pytest.mark.parametrize("kw", [dict(max_grad_norm=1.0, clip_grad_value=1.0), dict(max_grad_norm=0.0), dict(max_grad_norm=-1.0),
                                dict(max_grad_norm=float("nan")), dict(clip_grad_value=0), dict(clip_grad_value=-0.5),
                                dict(clip_grad_value=float("nan")), dict(max_grad_norm="1")])
def test_bad_settings_raise(kw):
    from vct_amd.trainer import CaptionTrainer, FusedAdam, build_optimizer
    m = _cpu_model()
    with pytest.raises(ValueError, match="max_grad_norm|clip_grad_value"):
        FusedAdam(m, **kw)
    with pytest.raises(ValueError, match="max_grad_norm|clip_grad_value"):
        build_optimizer(_tc(**kw), m)
    opt = torch.optim.Adam([m.flat_params], lr=1e-4)          # written into the group behind the factory's back: the trainer checks
    opt.param_groups[0].update(kw)
    with pytest.raises(ValueError, match="max_grad_norm|clip_grad_value"):
        CaptionTrainer(m, opt)


class _ActiveExchange:
    active, world, group = True, 2, None


def test_trainer_refuses_clipping_with_an_active_exchange():
    from vct_amd.trainer import CaptionTrainer, FusedAdam
    m = _cpu_model()
    for kw in (dict(max_grad_norm=1.0), dict(clip_grad_value=0.5)):
        with pytest.raises(NotImplementedError, match="gradient exchange"):
            CaptionTrainer(m, FusedAdam(m, **kw), exchange=_ActiveExchange())
    CaptionTrainer(m, FusedAdam(m), exchange=_ActiveExchange())       # without the settings: as before
    tr = CaptionTrainer(m, FusedAdam(m, max_grad_norm=1.0))
    assert tr.fuse_adam is False and tr.clipper is not None
    names, norms = tr.grad_norms()
    own = [n for n in m._ps.names if m._ps.offsets[n] + m._ps.params[n].numel() <= m.caption_param_end]
    assert names == own and norms.shape == (len(own),)
    # one segment per parameter, never the padding between them
    arr = (tr.clipper.table[0].numpy().view(np.int64).reshape(-1, 3))
    assert [(int(a), int(b)) for a, b, _ in arr] == [(m._ps.offsets[n], m._ps.offsets[n] + m._ps.params[n].numel()) for n in own]
    assert CaptionTrainer(m, FusedAdam(m)).grad_norms() is None and CaptionTrainer(m, FusedAdam(m, clip_grad_value=1.0)).last_grad_norm is None
