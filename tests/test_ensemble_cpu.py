"""Ensemble decoding without a GPU: tests/ensemble_ref.py against torch.log_softmax / torch.logsumexp, its checker against seeded
faults (each one rejected on its own), decode.Ensemble's constructor refusals and weight normalisation, and the refusals of
vct_ensemble_combine through the library (no device is touched: every refusal comes before any device use)."""
import ctypes
import math

import pytest
import torch

import ensemble_ref as ER

F64, F32, BF = ER.F64, ER.F32, ER.BF


# ---- the reference ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ER.MODES)
@pytest.mark.parametrize("n", [1, 2, 3, 8])
def test_reference_equals_torch(mode, n):
    rows, V = 3, 257
    xs, w = ER.members(rows, V, n, seed=11 + n), ER.weights(n, seed=n)
    out, bound = ER.combine(xs, w, mode)
    lps = torch.stack([torch.log_softmax(x.to(F64), 1) for x in xs])
    w64 = torch.tensor(ER.w32(w), dtype=F64).view(n, 1, 1)
    want = (w64 * lps).sum(0) if mode == "logp" else torch.logsumexp(lps + torch.log(w64), 0)
    torch.testing.assert_close(out, want, rtol=1e-12, atol=1e-12)
    assert bool((bound > 0).all()) and float(bound.max()) < 1e-2        # a bound, and one that still tells tokens apart
    if mode == "prob":                                 # the arithmetic mean is a distribution again (of mass sum w, the fp32 weights')
        mass = torch.full((rows,), math.fsum(ER.w32(w)), dtype=F64)
        torch.testing.assert_close(torch.exp(out).sum(1), mass, rtol=1e-12, atol=1e-12)


def test_reference_skips_zero_weights_and_confines_nan():
    rows, V = 3, 65
    xs = ER.members(rows, V, 3, seed=3, dtypes=(F32,))
    two, _ = ER.combine([xs[0], xs[2]], [0.25, 0.75], "prob")
    poisoned = torch.full_like(xs[1], float("nan"))
    for mode in ER.MODES:
        a, _ = ER.combine([xs[0], poisoned, xs[2]], [0.25, 0.0, 0.75], mode)
        b, _ = ER.combine([xs[0], xs[2]], [0.25, 0.75], mode)
        assert torch.equal(a, b)
    xs[0][1, 5] = float("nan")
    out, _ = ER.combine(xs, [0.5, 0.25, 0.25], "prob")
    assert bool(torch.isnan(out[1]).all()) and bool(torch.isfinite(out[[0, 2]]).all())
    assert bool(torch.isfinite(two).all())


def test_reference_shift_and_infinities():
    """One member near +80 where the other sits near -80: the log-probabilities of both are far below exp's underflow together, and
    the shift by A keeps the arithmetic mean finite; -inf in every member gives -inf."""
    x0, x1 = ER.shift_case(2, 33, seed=9)
    out, bound = ER.combine([x0, x1], [0.5, 0.5], "prob")
    assert bool(torch.isfinite(out[:, [0, 1, 2]]).all()) and float(out[:, 2].max()) < -150.0
    assert bool((out[:, 3] == float("-inf")).all())
    torch.testing.assert_close(out[:, 0], torch.full((2,), math.log(0.5), dtype=F64), rtol=0, atol=1e-9)
    out, _ = ER.combine([x0, x1], [0.5, 0.5], "logp")
    assert bool((out[:, 3] == float("-inf")).all()) and bool(torch.isfinite(out[:, :3]).all())


# ---- the checker ----------------------------------------------------------------------------------------------------------------------------
def _fault_case():
    rows, V = 3, 257
    xs = ER.members(rows, V, 3, seed=21)
    xs[1][:, 3] = float("-inf")          # the member of weight 0: multiplied instead of skipped, 0 * -inf is NaN
    xs[1][2, 9] = float("nan")
    return xs, [0.625, 0.0, 0.375]


@pytest.mark.parametrize("mode", ER.MODES)
def test_checker_accepts_the_float32_emulation(mode):
    xs, w = _fault_case()
    out, bound = ER.combine(xs, w, mode)
    assert ER.check("emulation", ER.emulate(xs, w, mode), out, bound) <= 1.0
    xs = ER.members(2, 30522, 4, seed=2)
    w = ER.weights(4, seed=5)
    out, bound = ER.combine(xs, w, mode)
    ER.check("emulation, V 30522", ER.emulate(xs, w, mode), out, bound)


@pytest.mark.parametrize("mode", ER.MODES)
@pytest.mark.parametrize("fault", ER.FAULTS)
def test_checker_rejects_every_seeded_fault(fault, mode):
    xs, w = _fault_case()
    out, bound = ER.combine(xs, w, mode)
    with pytest.raises(AssertionError):
        ER.check(fault, ER.emulate(xs, w, mode, fault=fault), out, bound)


# ---- decode.Ensemble: refusals before any device work, weights ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cpu_models():
    return ER.tiny_models("cpu")


def test_weight_normalisation(cpu_models):
    from vct_amd import decode
    assert decode.ENSEMBLE_MAX == 8
    assert decode.normalise_weights(None, 4) == [0.25] * 4 + [0.0] * 4
    assert decode.normalise_weights([2, 6], 2) == [0.25, 0.75] + [0.0] * 6
    assert decode.normalise_weights([0, 3.0, 0], 3) == [0.0, 1.0, 0.0] + [0.0] * 5
    w = decode.normalise_weights([0.1] * 7, 7)
    assert len(w) == 8 and abs(math.fsum(w) - 1.0) < 1e-15 and w[7] == 0.0
    a, b = cpu_models
    ens = decode.Ensemble([a, b], weights=[1, 3], mode="logprob")
    assert ens.weights == [0.25, 0.75] and ens._w.dtype == torch.float32 and ens._w.tolist() == [0.25, 0.75] + [0.0] * 6
    ens.set_weights([3, 1])
    assert ens.weights == [0.75, 0.25] and ens._w.tolist() == [0.75, 0.25] + [0.0] * 6
    assert decode.Ensemble([a]).weights == [1.0] and decode.Ensemble([a, b]).mode == "prob"
    assert ens.device == a.device and ens.cap_preprocessor is a.cap_preprocessor and ens.eval() is ens


def test_constructor_refusals(cpu_models, monkeypatch):
    from vct_amd import decode
    from encvar_ref import encvar_config
    from helpers import build_model
    a, b = cpu_models
    E = decode.Ensemble
    with pytest.raises(ValueError, match="members"):
        E([])
    with pytest.raises(ValueError, match="members"):
        E([a] * 9)
    with pytest.raises(ValueError, match="mode"):
        E([a, b], mode="mean")
    for bad in ([1.0], [1.0, 2.0, 3.0], [1.0, -0.5], [1.0, float("nan")], [float("inf"), 1.0], [0.0, 0.0]):
        with pytest.raises(ValueError, match="weights"):
            E([a, b], weights=bad)
        ens = E([a, b])
        with pytest.raises(ValueError, match="weights"):
            ens.set_weights(bad)
        assert ens.weights == [0.5, 0.5]
    other_vocab = build_model(encvar_config([48, 24]), 140, "cpu", torch.float32)
    with pytest.raises(ValueError, match="vocabulary"):
        E([a, other_vocab])
    one_stream = build_model(encvar_config([48]), ER.V_TINY, "cpu", torch.float32)
    with pytest.raises(ValueError, match="feature streams"):
        E([a, one_stream])
    for name in ("start_id", "end_id", "pad_id"):
        with monkeypatch.context() as mp:
            mp.setattr(b.cap_preprocessor, name, 77)
            with pytest.raises(ValueError, match="ids"):
                E([a, b])
    with monkeypatch.context() as mp:
        mp.setattr(b, "device", torch.device("meta"))
        with pytest.raises(ValueError, match="is on"):
            E([a, b])
    E([a, b])                                                             # (and the pair itself is accepted)
    feats = ER.tiny_batch(2, 0, "cpu")
    ens = E([a, b])
    for call in (lambda: ens.greedy_decode_ids(feats, None, 8, return_attn=True), lambda: ens.greedy_decode(feats, None, 8, return_attn=True),
                 lambda: ens.beam_decode_ids(feats, None, 3, 8, return_attn=True), lambda: ens.beam_decode(feats, None, 3, 8, return_attn=True)):
        with pytest.raises(ValueError, match="return_attn"):
            call()


# ---- the library's refusals ---------------------------------------------------------------------------------------------------------------------
def test_library_refusals_without_a_device():
    import __graft_entry__ as g
    g.build()
    from vct_amd import _lib
    lib = _lib.load()
    ARG, SHAPE = -1, -2
    assert lib.vct_ensemble_combine(None, None) == ARG
    raw = (ctypes.c_char * 256)()
    p = (ctypes.addressof(raw) + 15) & ~15

    def call(n=2, mode=0, rows=3, V=10, ld_all=16, ld_out=16, **kw):
        d = _lib.EnsembleDesc()
        d.n, d.mode, d.rows, d.V = n, mode, rows, V
        for m in range(max(0, min(n, 8))):
            d.dtype[m], d.x[m], d.ld[m] = _lib.F32, p, ld_all
        d.w, d.out, d.ld_out = p, p, ld_out
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(d, k)[v[0]] = v[1]
            else:
                setattr(d, k, v)
        return lib.vct_ensemble_combine(ctypes.byref(d), None)
    # every descriptor below also carries a refusal of the OTHER code further down the list of checks or none at all: a missing check
    # would show as the wrong code (or as a launch on host pointers), not pass silently
    for n in (0, -1, 9):
        assert call(n=n) == SHAPE
    assert call(mode=2) == ARG and call(mode=-1) == ARG
    assert call(w=None) == ARG and call(out=None) == ARG and call(x=(1, None)) == ARG
    assert call(dtype=(0, 2)) == ARG and call(dtype=(1, -1)) == ARG
    assert call(rows=0) == SHAPE and call(rows=-3) == SHAPE and call(V=0) == SHAPE and call(V=-1) == SHAPE
    assert call(V=17) == SHAPE and call(ld=(1, 9)) == SHAPE and call(ld_out=9) == SHAPE
    assert call(mode=2, rows=0) == ARG and call(x=(0, None), V=0) == ARG       # VCT_E_ARG comes first
    assert _lib.C_CONSTANTS["VCT_ENSEMBLE_MAX"] == 8 and _lib.C_CONSTANTS["VCT_ENS_PROB"] == 0 and _lib.C_CONSTANTS["VCT_ENS_LOGP"] == 1
    assert _lib.ABI_VERSION == 16
