"""The video-text matching task (train.task "match" / "cross") without a GPU: the float64 restatement of the head
(tests/matching_ref.py) against the reference's recorded numbers (tests/golden/matching_*.npz, tools/make_golden_matching.py), the
state-dict surface in every temperature form, the flat layout and the optimizer's range per task, every refusal, and the argument
errors of the new entry points."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import matching_ref as R
from helpers import GOLDEN, build_model, load_golden, model_config_of
from hmm_ref import hmm_config, hmm_params

V = 131
CASES = ["P", "L", "N", "W_fixed", "W_learned", "X"]


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def _cpu_model(kind="CSL", form="none", text_dim=48, shapes=(48,), tau=0.5, matching="block", **kw):
    blk = R.matching_block(kind, form, tau) if matching == "block" else matching
    mc = R.matching_config(list(shapes), text_dim, blk, **kw)
    return build_model(mc, V, "cpu", torch.float32, R.matching_params(mc, V, 5)), mc


# ---- the restatement against the reference ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_the_fixture(case):
    z = load_golden(f"matching_{case}.npz")
    mc = model_config_of(z)
    p = R.matching_params(mc, V, int(z["param_seed"]))
    kind, temp = mc["matching"]["matching_loss"], R.temp_of(z)
    W, b = p.get("matching.v_proj.weight"), p.get("matching.v_proj.bias")
    out = R.head_with_proj(z["text_feats"], z["agg"], W, b, kind, temp)
    cross = str(z["task"]) == "cross"
    w = 1.0 - mc["loss_beta"] if cross else 1.0            # the share of the match loss in what was backpropagated
    assert abs(out["loss"] - float(z["match_loss"] if cross else z["loss"])) < 1e-6 * abs(out["loss"])
    assert _rel(out["vid"], z["vid"]) < 1e-6 and _rel(out["sim"], z["sim"]) < 1e-6
    assert _rel(w * out["dagg"], z["dagg"]) < 1e-6
    if W is not None:
        assert _rel(w * out["dW"], z["grad/matching.v_proj.weight"]) < 1e-6
        assert _rel(w * out["db"], z["grad/matching.v_proj.bias"]) < 1e-6
    if mc["matching"]["enable_tem"] and mc["matching"].get("temperature") is None:
        got, want = w * out["dtemp"], float(z["grad/matching.loss_fn.temperature"][0])
        assert abs(got - want) < 1e-6 * w * out["dtemp_abs"]
    else:
        assert "grad/matching.loss_fn.temperature" not in z.files
    if cross:
        assert abs(float(z["loss"]) - (mc["loss_beta"] * float(z["cap_loss"]) + w * float(z["match_loss"]))) < 1e-6 * float(z["loss"])
        assert json.loads(str(z["no_grad"])) == []
    else:
        none = json.loads(str(z["no_grad"]))
        assert none and all(k.startswith("cap_decoder.") for k in none)
        assert not any(k.startswith("grad/cap_decoder.") for k in z.files)


def test_argument_order_matters_for_the_dual_softmax():
    """CSL is symmetric in (text, vid); CSL_WDS is not: its prior is a softmax over the TEXT index."""
    rng = np.random.default_rng(0)
    t, v = rng.standard_normal((5, 16)), rng.standard_normal((5, 16))
    assert abs(R.head(t, v, "CSL", 0.07, False)["loss"] - R.head(v, t, "CSL", 0.07, False)["loss"]) < 1e-12
    assert abs(R.head(t, v, "CSL_WDS", 0.5, False)["loss"] - R.head(v, t, "CSL_WDS", 0.5, False)["loss"]) > 1e-3


@pytest.mark.parametrize("kind,temp", [("CSL", None), ("CSL", 0.07), ("CSL_WDS", 0.5), ("CSL_WDS", 0.05)])
def test_restatement_gradients_by_finite_differences(kind, temp):
    rng = np.random.default_rng(3)
    t, v = rng.standard_normal((4, 8)), rng.standard_normal((4, 8))
    out = R.head(t, v, kind, temp)
    eps = 1e-6
    num = np.zeros_like(v)
    for i in range(v.shape[0]):
        for k in range(v.shape[1]):
            a, b = v.copy(), v.copy()
            a[i, k] += eps
            b[i, k] -= eps
            num[i, k] = (R.head(t, a, kind, temp, False)["loss"] - R.head(t, b, kind, temp, False)["loss"]) / (2 * eps)
    assert _rel(out["dvid"], num) < 1e-6
    if temp is not None:
        nt = (R.head(t, v, kind, temp + eps, False)["loss"] - R.head(t, v, kind, temp - eps, False)["loss"]) / (2 * eps)
        assert abs(out["dtemp"] - nt) < 1e-6 * out["dtemp_abs"]


def test_single_pair_has_zero_loss_and_gradients():
    rng = np.random.default_rng(1)
    for kind, temp in (("CSL", None), ("CSL", 2.5), ("CSL_WDS", 0.5)):
        out = R.head(rng.standard_normal((1, 8)), rng.standard_normal((1, 8)), kind, temp)
        assert out["loss"] == 0.0 and not np.abs(out["dvid"]).max() > 1e-16 and (temp is None or out["dtemp"] == 0.0)


# ---- construction, state dict, flat layout -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("text_dim", [48, 64])
@pytest.mark.parametrize("form", ["none", "fixed", "learned"])
@pytest.mark.parametrize("kind", ["CSL", "CSL_WDS"])
def test_state_dict_keys_in_every_temperature_form(kind, form, text_dim):
    with open(os.path.join(GOLDEN, "matching_state_keys.json")) as f:
        want = json.load(f)[f"{kind}/{form}/text{text_dim}"]
    if kind == "CSL_WDS" and form == "none":
        with pytest.raises(ValueError, match="temperature"):
            _cpu_model(kind, form, text_dim)
        return
    m, _ = _cpu_model(kind, form, text_dim)
    got = {k: list(v.shape) for k, v in m.state_dict().items() if k.startswith("matching.")}
    assert got == want
    lf = m.matching.loss_fn
    assert lf.learned == (form == "learned") and (lf.temperature is None) == (form == "none")
    if form == "fixed":
        assert not isinstance(lf.temperature, torch.nn.Parameter) and float(lf.temperature) == 0.5
    if form == "learned":
        assert float(lf.temperature) == 1.0 and lf.temperature.dtype == torch.float32


def test_flat_layout_ends_with_matching_and_buckets_tile_it():
    m, _ = _cpu_model("CSL", "learned", 48, shapes=(48, 24))
    names = m._ps.names
    tail = [n for n in names if n.startswith("matching.")]
    assert tail == ["matching.v_proj.weight", "matching.v_proj.bias", "matching.loss_fn.temperature"] and names[-3:] == tail
    assert m.caption_param_end == m._ps.offsets["matching.v_proj.weight"]
    buckets = m.grad_buckets()
    assert buckets[0][0] == 0 and buckets[-1][1] == m._ps.total
    assert all(buckets[i][1] == buckets[i + 1][0] for i in range(len(buckets) - 1))
    # the learned temperature aliases the flat buffer like every other parameter
    assert m.matching.loss_fn.temperature.data_ptr() == m.flat_params.data_ptr() + 4 * m._ps.offsets["matching.loss_fn.temperature"]


def test_mode_flags_follow_the_reference():
    m, _ = _cpu_model("CSL", "learned", 48)
    flags = {}
    for task in ("caption", "match", "cross"):
        m.mode(task)
        flags[task] = (all(p.requires_grad for p in m.cap_decoder.parameters()), all(p.requires_grad for p in m.matching.parameters()),
                       any(p.requires_grad for p in m.cap_decoder.parameters()), all(p.requires_grad for p in m.video_encoder.parameters()))
    assert flags == {"caption": (True, False, True, True), "match": (False, True, False, True), "cross": (True, True, True, True)}


def test_optimizer_range_per_task():
    from vct_amd.trainer import FusedAdam
    from vct_amd.trainer.optim import owned_range
    m, _ = _cpu_model("CSL", "learned", 48)
    total, enc0, cap_end = m._ps.total, m.encoder_param_begin, m.caption_param_end
    assert 0 < enc0 < cap_end < total
    assert owned_range(m, None) == owned_range(m, "caption") == (0, cap_end)
    assert owned_range(m, "match") == (enc0, total) and owned_range(m, "cross") == (0, total)
    with pytest.raises(ValueError):
        owned_range(m, "other")
    for task, want in (("caption", (0, cap_end)), ("match", (enc0, total)), ("cross", (0, total))):
        m.mode(task)
        opt = FusedAdam(m, lr=1e-4)
        assert (opt.begin, opt.end) == want and opt.task == task
        # the token-embedding skip range lies outside the match task's range and inside the others'
        assert (opt.skip[1] <= opt.begin) == (task == "match")


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def _batch(B=3, dim=48, shapes=(48,), Ts=(5,)):
    from mm_ref import mm_batch
    feats, masks, ids = mm_batch(B, Ts, shapes, 7, V, seed=9)
    return ([torch.from_numpy(f) for f in feats], [torch.from_numpy(k) for k in masks], torch.from_numpy(ids),
            torch.randn(B, dim))


class _ActiveExchange:
    active, world, group = True, 2, None


@pytest.mark.parametrize("task", ["match", "cross"])
def test_refusals(task):
    from vct_amd.trainer import CaptionTrainer
    feats, masks, ids, text = _batch()
    # the hierarchical encoder: its agg_feats is [B]
    mc = hmm_config([48, 24], [2, 1])
    hm = build_model(mc, V, "cpu", torch.float32, hmm_params(mc, V, 5))
    hm.mode(task)
    f2, m2, i2, t2 = _batch(dim=hm.text_encoder.dim, shapes=(48, 24), Ts=(5, 3))
    with pytest.raises(NotImplementedError, match="hmme"):
        hm(f2, m2, i2, text_feats=t2)
    with pytest.raises(NotImplementedError, match="hmme"):
        CaptionTrainer(hm, torch.optim.Adam([hm.flat_params], lr=1e-4))
    # no matching head
    nm, _ = _cpu_model(matching=None, text_dim=64)
    nm.mode(task)
    with pytest.raises(ValueError, match="matching"):
        nm(feats, masks, ids, text_feats=text)
    # recorded executors and the gradient exchange
    m, _ = _cpu_model("CSL", "fixed", 48)
    m.mode(task)
    opt = torch.optim.Adam([m.flat_params], lr=1e-4)
    for kw in (dict(use_graph=True), dict(launch_list=True), dict(exchange=_ActiveExchange())):
        with pytest.raises(NotImplementedError, match="eager|single-process"):
            CaptionTrainer(m, opt, **kw)
    # the optimizer was built for another task
    tr = CaptionTrainer(m, opt)
    m.mode("caption")
    with pytest.raises(ValueError, match="optimizer was built"):
        tr.step(feats[0], masks[0], ids, text)
    m.mode(task)
    with pytest.raises(ValueError, match="text_feats"):
        tr.step(feats[0], masks[0], ids)
    # text features of the wrong shape, dtype, device; no backend installed
    for bad in (text[:, :40], text[:2], text.double(), text.to("meta"), text.numpy()):
        with pytest.raises(ValueError, match="text_feats"):
            m(feats, masks, ids, text_feats=bad)
    with pytest.raises(RuntimeError, match="text_feats"):
        m(feats, masks, ids)
    m.text_encoder.backend = lambda caps: torch.zeros(len(caps), 7)
    with pytest.raises(ValueError, match="backend"):
        m(feats, masks, ids)
    # a batch beyond the kernels' range, from Python
    fb, mb, ib, tb = _batch(B=257)
    with pytest.raises(ValueError, match="256"):
        m(fb, mb, ib, text_feats=tb)


def test_unsupported_text_dimension_and_epoch_loops_refuse_in_python():
    from vct_amd.evaluate import val_epoch
    from vct_amd.trainer import train_epoch
    with pytest.raises(ValueError, match="multiples of 4"):
        _cpu_model("CSL", "fixed", 50)
    with pytest.raises(ValueError, match="multiples of 4"):
        _cpu_model("CSL", "fixed", 1028)
    with pytest.raises(ValueError, match="CSL"):
        _cpu_model(matching={"enable_tem": False, "matching_loss": "other"})
    m, _ = _cpu_model("CSL", "fixed", 48)
    with pytest.raises(ValueError, match="unknown task"):
        train_epoch(m, None, [], mode="other")
    with pytest.raises(ValueError, match="unknown task"):
        val_epoch(m, [], mode="other")


def test_no_text_model_import():
    """The text side is a user-installed callable: nothing here imports clip or transformers."""
    import sys
    import vct_amd.model  # noqa: F401
    for name in ("Matching", "MMT4Caption"):       # (the package re-exports classes under the modules' names)
        src = open(sys.modules["vct_amd.model." + name].__file__).read()
        assert "import clip" not in src and "import transformers" not in src and "from transformers" not in src


# ---- the C entry points ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from vct_amd import _lib
    return _lib.load()


def test_entry_points_validate_arguments(lib):
    from vct_amd import _lib
    assert lib.vct_match_loss(None, None) == -1
    buf = (ctypes.c_float * 4096)()
    p = ctypes.addressof(buf)
    p = (p + 15) // 16 * 16

    def desc(**kw):
        d = _lib.MatchLossDesc()
        d.B, d.Dt, d.loss_kind, d.temp_kind = 4, 16, 0, 0
        d.text = d.vid = d.loss = d.workspace = p
        d.ld_text = d.ld_vid = 16
        d.workspace_bytes = 1 << 14
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    assert lib.vct_match_loss(desc(text=None), None) == -1
    assert lib.vct_match_loss(desc(loss=None), None) == -1 and lib.vct_match_loss(desc(workspace=None), None) == -1
    assert lib.vct_match_loss(desc(loss_kind=2), None) == -1 and lib.vct_match_loss(desc(temp_kind=3), None) == -1
    assert lib.vct_match_loss(desc(loss_kind=1), None) == -1                       # CSL_WDS without a temperature
    assert lib.vct_match_loss(desc(temp_kind=2, temp=p), None) == -1               # CSL does not divide
    assert lib.vct_match_loss(desc(temp_kind=1), None) == -1                       # a kind without its scalar
    assert lib.vct_match_loss(desc(temp=p), None) == -1                            # a scalar without a kind
    for B, Dt in ((0, 16), (257, 16), (4, 18), (4, 0), (4, 1028)):
        assert lib.vct_match_loss(desc(B=B, Dt=Dt, ld_text=1028, ld_vid=1028), None) == -2
    assert lib.vct_match_loss(desc(ld_vid=8), None) == -2
    assert lib.vct_match_loss(desc(ld_text=18), None) == -3 and lib.vct_match_loss(desc(text=p + 4), None) == -3
    assert lib.vct_match_loss(desc(workspace_bytes=64), None) == -4
    # the workspace query: 0 outside the range, monotone in B inside it
    assert lib.vct_match_loss_workspace_bytes(0, 16) == 0 and lib.vct_match_loss_workspace_bytes(257, 16) == 0
    assert lib.vct_match_loss_workspace_bytes(4, 18) == 0 and lib.vct_match_loss_workspace_bytes(4, 1028) == 0
    sizes = [lib.vct_match_loss_workspace_bytes(B, 512) for B in range(1, 257)]
    assert all(a < b for a, b in zip(sizes, sizes[1:])) and sizes[0] >= 4 and sizes[-1] >= 4 * 256 * 256
    # the aggregation rows, the scale and the mix
    assert lib.vct_match_agg_fwd(None, None) == -1 and lib.vct_match_agg_bwd(None, None) == -1
    a = _lib.MatchAggDesc()
    a.dtype, a.B, a.Te, a.d = 0, 2, 3, 8
    assert lib.vct_match_agg_fwd(a, None) == -1 and lib.vct_match_agg_bwd(a, None) == -1        # null operands
    a.mem = a.agg = a.dagg = a.dmem = p
    a.dtype = 5
    assert lib.vct_match_agg_fwd(a, None) == -1
    a.dtype, a.B = 0, 0
    assert lib.vct_match_agg_fwd(a, None) == -2
    a.B, a.d = 2, 6
    assert lib.vct_match_agg_bwd(a, None) == -3
    a.d, a.beta = 8, 1.5
    assert lib.vct_match_agg_bwd(a, None) == -1
    assert lib.vct_scale(None, 8, 0.5, None) == -1 and lib.vct_scale(p, -1, 0.5, None) == -2 and lib.vct_scale(p + 4, 8, 0.5, None) == -3
    assert lib.vct_scale(p, 0, 0.5, None) == 0
    assert lib.vct_axpby(None, p, 1.0, None, 0.0, 1, None) == -1 and lib.vct_axpby(p, None, 1.0, None, 0.0, 1, None) == -1
    assert lib.vct_axpby(p, p, 1.0, None, 0.0, -1, None) == -2 and lib.vct_axpby(p, p, 1.0, None, 0.0, 0, None) == 0


def test_python_wrappers_turn_shape_codes_into_value_errors(lib):
    from vct_amd import ops
    with pytest.raises(ValueError, match="outside the kernels' range"):
        ops.match_loss_workspace_bytes(257, 512)
    with pytest.raises(ValueError, match="outside the kernels' range"):
        ops.match_loss_workspace_bytes(8, 1028)
    assert ops.match_loss_workspace_bytes(256, 1024) >= 4 * 256 * 256
