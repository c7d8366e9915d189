"""CPU checks of tests/frontend_ref.py, the fp64 references, bounds and checkers of tests/test_frontend_kernels_gpu.py (no GPU):
  * the front-end references against torch autograd through mean / amax / cat / nn.LayerNorm / nn.Embedding in all eight option
    combinations, against oracle/vct_oracle.py's front end for the single-stream form, the tie rule against torch's max-pool backward,
    cast_rne against torch.Tensor.to(torch.bfloat16) over the full pattern set, the dropout mask against layer_ss_ref.drop_mult;
  * a CORRECT float32 emulation of every operation stays inside the derived bounds at every entry of frontend_ref.SHAPES in both types
    (the worst |delta| / bound is printed and must be below 1);
  * every fault of frontend_ref.FAULTS is rejected by the checker the GPU file uses for it, at the shape named for it;
  * the random inputs have no accidental ties in the max columns and no bound is larger than its reference's magnitude in more than 1 % of
    the elements: a bound can never become vacuous;
  * the refusals that need no device return the codes include/vct_hip.h names (the library loads without a GPU)."""
import ctypes

import numpy as np
import pytest
import torch

import frontend_ref as F
import layer_ss_ref as LR
import vct_oracle as O

F64, F32, BF = F.F64, F.F32, F.BF
Z = F.SHAPES
TYPES = pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
E_ARG, E_SHAPE = -1, -2


# ---- the references against independent statements ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("agg,learned,norm", F.COMBOS)
@pytest.mark.parametrize("Ts", [(5, 3, 2), (4,)])
def test_front_reference_is_autograd(agg, learned, norm, Ts):
    B, d = 3, 12
    c = F.Case(F32, Ts, B, d, seed=41)
    n, S = c.n, c.S
    drop = (F.SEED, F.SITE, 0.3) if norm else None
    us = [u.double().view(B, t, d).requires_grad_(True) for u, t in zip(c.us, Ts)]
    emb = torch.nn.Embedding(c.emb_rows, d).double()
    emb.weight.data = torch.nan_to_num(c.emb_w.double(), nan=0.0)
    modal = None
    if n > 1:
        modal = torch.nn.Embedding(c.n_labels, d).double()
        modal.weight.data = torch.nan_to_num(c.modal_w.double(), nan=0.0)
    ln = torch.nn.LayerNorm(d, eps=1e-5).double()
    ln.weight.data, ln.bias.data = c.gamma.double(), c.beta.double()
    blocks = []
    for u in us:
        a = u.mean(1, keepdim=True) if agg == "avg" else u.amax(1, keepdim=True)
        blocks.append(torch.cat([a, u], 1))
    add = emb(c.tidx.long()) if learned else c.temp.double()
    if n > 1:
        add = add + modal(c.labels.long())
    pre = torch.cat(blocks, 1) + add[None]
    pre.retain_grad()
    mask = F.drop_mask(B * S, d, drop) if norm else None
    x0 = ln(pre).view(B * S, d) * mask if norm else pre.view(B * S, d)
    x0.backward(c.dx.double())
    r = F.reference(c, agg, learned, norm, drop)
    assert torch.allclose(r["x0"], x0.detach(), rtol=1e-11, atol=1e-12)
    # behind the norm the backward's operands are the statistics ROUNDED to fp32 (what the kernel is handed): 2^-24 relative on each
    tol = dict(rtol=1e-5, atol=1e-6) if norm else dict(rtol=1e-9, atol=1e-12)
    for i, u in enumerate(us):
        assert torch.allclose(r["du"][i], u.grad.view(-1, d), **tol), i
    assert torch.allclose(r["dpre_ref"], pre.grad.view(-1, d), **tol)
    if n > 1:
        assert torch.allclose(r["d_modal"], modal.weight.grad, **tol)
    if learned:
        assert torch.allclose(r["d_emb"], emb.weight.grad, **tol)
        assert bool((r["d_emb"][r["emb_cnt"] == 0] == 0).all()) and int((r["emb_cnt"] > 0).sum()) == int(c.emb_read.sum())
    if norm:
        ws = r["ws"].view(B * n, 2, d).sum(0)
        assert torch.allclose(ws[0], ln.weight.grad, **tol) and torch.allclose(ws[1], ln.bias.grad, rtol=1e-9, atol=1e-12)
        pr = pre.detach().view(-1, d)
        assert torch.allclose(r["mean"], pr.mean(1), rtol=1e-12) and torch.allclose(r["rstd"], 1 / torch.sqrt(pr.var(1, unbiased=False) + 1e-5), rtol=1e-12)
    key = torch.cat([torch.cat([torch.zeros(B, 1, dtype=torch.uint8), m], 1) for m in c.masks], 1)
    assert torch.equal(r["key_pad"], key)


def test_single_stream_reference_is_the_oracle():
    B, T, d = 3, 6, 16
    c = F.Case(F32, (T,), B, d, seed=42)
    p = {O.ENC + "unify.0.weight": np.eye(d), O.ENC + "unify.0.bias": np.zeros(d), O.ENC + "temp_emb.pe": O.encoder_pos_table(512, d)}
    feats = c.us[0].double().view(B, T, d).numpy()
    z, cache = O.encoder_frontend(p, feats, dt=np.float64)
    pe_rows = torch.from_numpy(O.temporal_encoding_rows(p[O.ENC + "temp_emb.pe"], T))
    assert float(pe_rows[0].abs().sum()) == 0.0
    f = F.front_fwd(c.us, None, F.add_rows(c.S, d, temp=pe_rows), "avg", (T,), B)
    assert np.allclose(f["pre"].numpy(), z, rtol=1e-13, atol=1e-14)
    dz = c.dx.double().view(B, T + 1, d).numpy()
    g = O.encoder_frontend_bwd(dz, cache, p, dt=np.float64)
    r = F.front_bwd(c.dx.double(), (T,), B, "avg")
    assert np.allclose(r["du"][0].sum(0).numpy(), g[O.ENC + "unify.0.bias"], rtol=1e-12)
    assert np.allclose(r["du"][0].numpy().T @ feats.reshape(-1, d), g[O.ENC + "unify.0.weight"], rtol=1e-11, atol=1e-12)


def test_tie_rule_is_max_pool_backward():
    t = Z["ties"]
    c = F.Case(F32, t["Ts"], t["B"], t["d"], seed=10, ties=True)
    f = F.front_fwd(c.us, c.masks, c.add_rows(False), "max", c.Ts, c.B)
    for i, T in enumerate(c.Ts):
        x = c.us[i].double().view(c.B, T, c.d).permute(0, 2, 1).contiguous().requires_grad_(True)
        torch.nn.functional.adaptive_max_pool1d(x, 1).sum().backward()
        assert torch.equal(x.grad.argmax(2), f["arg"][i]) and float(x.grad.sum()) == c.B * c.d
        u = c.us[i].view(c.B, T, c.d)
        ties = (u == u.max(1, keepdim=True).values).sum(1)
        if T >= 3:          # two leading rows, two trailing rows, three rows, two rows apart; no other column ties
            assert ties[:, :4].tolist() == [[2, 2, 3, 2]] * c.B and bool((ties[:, 4:] == 1).all())
            assert f["arg"][i][:, :4].tolist() == [[0, T - 2, 0, 1]] * c.B


def test_cast_reference_is_torch_rounding():
    pat = F.cast_patterns()
    assert pat.size == 393216
    want = F.bf_bits(F.bits_f32(pat).to(BF))
    got = F.cast_rne(pat)
    nan = (pat & 0x7FFFFFFF) > 0x7F800000
    assert np.array_equal(got[~nan], want[~nan]) and bool(F.is_nan16(got[nan]).all()) and bool(F.is_nan16(want[nan]).all())
    assert np.array_equal(F.emulate_cast(pat), got)
    for word, bits in ((0x3F808000, 0x3F80), (0x3F818000, 0x3F82), (0x3FFF8000, 0x4000), (0x7F7F8000, 0x7F80), (0x00008000, 0x0000),
                       (0x00018000, 0x0002), (0x80000000, 0x8000), (0x007FFFFF, 0x0080), (0xFF7FFFFF, 0xFF80), (0x7F800001, 0x7FC0)):
        assert int(F.cast_rne(np.array([word]))[0]) == bits, hex(word)


def test_mask_reference_is_the_counter_hash():
    B, S, d = 2, 8, 72
    for p in Z["drop_p"]:
        m = F.drop_mask(B * S, d, (F.SEED, F.SITE, p))
        want = LR.drop_mult(F.SEED, F.SITE, p, np.arange(B * S * d)).reshape(B * S, d)
        assert np.array_equal(m.numpy(), want) and 0 < int((m == 0).sum()) < m.numel()
    assert bool((F.drop_mask(3, 8, (F.SEED, F.SITE, 0.0)) == 1).all())


def test_mix_and_gather_references():
    B, S, d = 2, 5, 8
    take = torch.tensor([1, 0, 1, 0, 0], dtype=torch.uint8)
    y, x0 = F.rnd((B * S, d), 1).double().requires_grad_(True), F.rnd((B * S, d), 2).double().requires_grad_(True)
    x = torch.where(take.bool().repeat(B)[:, None], y, x0)
    dx = F.rnd((B * S, d), 3)
    x.backward(dx.double())
    assert torch.equal(F.mix_fwd(y.detach(), x0.detach(), take, B, S), x.detach())
    dy, acc = F.mix_bwd(dx, take, torch.full((B * S, d), F.NAN), B, S, init=True)
    assert torch.equal(dy.double(), y.grad) and torch.equal(acc.double(), x0.grad)
    dy2, acc2 = F.mix_bwd(dx, take, acc, B, S)
    assert torch.equal(acc2, torch.where(take.bool().repeat(B)[:, None], acc, acc + dx))
    store, offs, idx = F.gather_case(6, 3, 3, zero="middle")
    out, mask = F.gather_pad(store, offs, idx, 3)
    assert not bool(torch.isnan(out).any()) and mask.tolist() == [[0, 0, 0], [0, 1, 1], [1, 1, 1]]
    assert torch.equal(out[0], store[:3].double()) and torch.equal(out[1, 0], store[3].double()) and float(out[2].abs().sum()) == 0.0
    store, offs, idx = F.gather_case(4, 2, 3, zero="last")
    assert int(offs[int(idx[-1])]) == store.shape[0] and int(offs[-1]) == store.shape[0]


# ---- the emulation stays inside every bound --------------------------------------------------------------------------------------------------------
@TYPES
def test_emulation_inside_every_bound_front(dtype, capsys):
    worst = 0.0
    for tag, c, combos, p, exact in F.ex_cases(dtype):
        for agg, learned, norm in combos:
            ref = F.reference(c, agg, learned, norm, F.drop_of(p))
            got = F.emulate_front(c, agg, learned, norm, F.drop_of(p))
            worst = max(worst, F.judge(f"{tag} {agg} learned={learned} norm={norm}", got, ref, c, agg, norm, exact))
    for tag, c, exact, _ in F.mm_cases(dtype):
        worst = max(worst, F.judge(f"mm {tag}", F.emulate_front(c, "avg", False, False), F.reference(c, "avg", False, False), c, "avg", False, exact))
    for tag, c in F.single_cases(dtype):
        worst = max(worst, F.judge(f"single {tag}", F.emulate_front(c, "avg", False, False), F.reference(c, "avg", False, False), c, "avg", False))
    capsys.readouterr()
    with capsys.disabled():
        print(f"\n[front] emulation, {dtype}: worst |delta| / bound = {worst:.3f}")
    assert 0.0 < worst <= 1.0


@TYPES
def test_emulation_inside_every_bound_movers(dtype):
    for B, S, d in Z["mix"][dtype]:
        takes = [torch.zeros(S, dtype=torch.uint8), torch.ones(S, dtype=torch.uint8), (torch.arange(S) % 2).to(torch.uint8)]
        dxs = [F.rnd((B * S, d), 60 + k, 1.0, dtype) for k in range(3)]
        acc = torch.full((B * S, d), F.NAN)
        acc_e = acc.clone()
        for k, take in enumerate(takes):                                # a three-layer chain, top layer first
            _, acc = F.mix_bwd(dxs[k], take, acc, B, S, init=k == 0)
            _, acc_e = F.emulate_mix_bwd(dxs[k], take, acc_e, B, S, init=k == 0)
        F.check_exact("mix chain acc", acc_e, acc)
        v, e = F.mix_close(dxs[0], acc)
        F.check_elem("mix dx0", (acc + dxs[0].float()).to(dtype), v, F.R.bound(v, e, dtype))
    for E in Z["gather_E"]:
        for B, Tmax in Z["gather_BT"]:
            for zero in ("none", "middle", "last"):
                store, offs, idx = F.gather_case(E, B, Tmax, zero=zero)
                ref, mask = F.gather_pad(store, offs, idx, Tmax)
                got, gm = F.emulate_gather(store, offs, idx, Tmax, dtype)
                assert torch.equal(mask, gm)
                if dtype == F32:
                    F.check_exact("gather", got, ref, F32)
                else:
                    F.check_bits("gather bf16", F.bf_bits(got), F.cast_rne(F.f32_bits(ref.to(F32))))
    for r, c in Z["transpose"]:
        src = F.bits_bf(np.arange(r * c, dtype=np.uint16) * 251 + 0x7F00).view(r, c)
        F.check_bits("transpose", F.bf_bits(F.emulate_transpose(src)), F.bf_bits(F.transpose(src)))


# ---- every fault is rejected -------------------------------------------------------------------------------------------------------------------------
def _front_fault(fault, dtype):
    """(Case, agg, learned, norm, p) of the shape named for the fault."""
    r, w, t, o = Z["ex_regs"], Z["lane_wrap"], Z["ties"], Z["oob"]
    regs = lambda **kw: F.Case(dtype, r["Ts"], r["B"], 8, seed=70, **kw)
    wrap = lambda **kw: F.Case(dtype, w["Ts"], w["B"], w["d"], seed=71, **kw)
    return {
        "avg_divides_by_T_plus_1": lambda: (regs(), "avg", False, False, None),
        "avg_drops_last_frame": lambda: (regs(), "avg", False, False, None),
        "temporal_row_shifted": lambda: (regs(), "avg", False, False, None),
        "agg_row_takes_frame_label": lambda: (regs(), "max", True, False, None),                 # n_labels = 2n
        "max_credits_last_tie": lambda: (F.Case(dtype, t["Ts"], t["B"], t["d"], seed=10, ties=True), "max", False, False, None),
        "share_not_divided": lambda: (regs(), "avg", True, False, None),
        "modal_drops_past_64": lambda: (wrap(), "avg", False, False, None),                      # B * cnt = 68 .. 102
        "emb_once_per_reader": lambda: (wrap(), "avg", True, False, None),                       # the four aggregation rows share row 0
        "emb_unread_unwritten": lambda: (regs(), "avg", True, False, None),
        "oob_label_clamped": lambda: (F.Case(dtype, o["Ts"], o["B"], o["d"], seed=7, oob=True), "avg", False, False, None),
        "one_pass_variance": lambda: (F.Case(dtype, r["Ts"], r["B"], 8, seed=17, big_mean=True), "avg", False, True, None),
        "drop_counter_row_in_stream": lambda: (F.Case(dtype, r["Ts"], r["B"], 72, seed=80), "avg", False, True, 0.5),
        "key_pad_agg_first_mask": lambda: (wrap(), "avg", False, False, None),
    }[fault]()


@TYPES
@pytest.mark.parametrize("fault", [k for k, v in F.FAULTS.items() if v == "front"])
def test_front_fault_is_rejected(fault, dtype):
    c, agg, learned, norm, p = _front_fault(fault, dtype)
    ref = F.reference(c, agg, learned, norm, F.drop_of(p))
    assert F.judge("correct", F.emulate_front(c, agg, learned, norm, F.drop_of(p)), ref, c, agg, norm) <= 1.0
    with pytest.raises(AssertionError):
        F.judge(fault, F.emulate_front(c, agg, learned, norm, F.drop_of(p), fault=fault), ref, c, agg, norm)


@TYPES
def test_mover_faults_are_rejected(dtype):
    store, offs, idx = F.gather_case(6, 3, 3, zero="none")
    ref, _ = F.gather_pad(store, offs, idx, 3)
    with pytest.raises(AssertionError):
        F.check_exact("pad_keeps_row_0", F.emulate_gather(store, offs, idx, 3, F32, fault="pad_keeps_row_0")[0], ref, F32)
    pat = F.cast_patterns()
    for fault in ("cast_truncates", "cast_no_exponent_carry"):
        with pytest.raises(AssertionError):
            F.check_bits(fault, F.emulate_cast(pat, fault), F.cast_rne(pat), nan_class=True)
    src = F.bits_bf(np.arange(7 * 9, dtype=np.uint16) + 0x3F80).view(7, 9)
    with pytest.raises(AssertionError):
        F.check_bits("transpose_drops_tail", F.bf_bits(F.emulate_transpose(src, "transpose_drops_tail")), F.bf_bits(F.transpose(src)))
    B, S, d = 3, 5, 72
    take = (torch.arange(S) % 2).to(torch.uint8)
    dx, acc = F.rnd((B * S, d), 1, 1.0, dtype), F.rnd((B * S, d), 2)
    with pytest.raises(AssertionError):
        F.check_exact("mix_accumulates_continuing", F.emulate_mix_bwd(dx, take, acc, B, S, fault="mix_accumulates_continuing")[1],
                      F.mix_bwd(dx, take, acc, B, S)[1])
    assert sorted(F.FAULTS) == sorted(set(F.FAULTS)) and len(F.FAULTS) == 18


# ---- conditions on the inputs: no accidental ties, no vacuous bound ---------------------------------------------------------------------------------
@TYPES
def test_inputs_have_no_accidental_ties_and_no_bound_is_vacuous(dtype, capsys):
    """Per kind of output, over every case of the table: the share of elements whose bound exceeds the reference's own magnitude."""
    over, total = {}, {}
    for tag, c, combos, p, exact in F.ex_cases(dtype):
        for i, T in enumerate(c.Ts):
            u = c.us[i].view(c.B, T, c.d)
            ties = (u == u.max(1, keepdim=True).values).sum(1)
            seeded = tag == "ties" and T >= 2
            assert bool((ties[:, 4 if seeded else 0:] == 1).all()), (tag, i)
        if exact:
            continue                                              # integer dx: sums that are exactly zero; judged bit for bit
        for agg, learned, norm in combos:
            ref = F.reference(c, agg, learned, norm, F.drop_of(p))
            pairs = [("x0", ref["x0"], ref["b_x0"])] + [("du", v, b) for v, b in zip(ref["du"], ref["b_du"])]
            pairs += [(k, ref[k], ref["b_" + k]) for k in ("mean", "rstd", "dpre") if k in ref]
            if "ws" in ref:
                pairs.append(("param_ws", ref["ws"], ref["b_ws"]))
            if "d_modal" in ref:
                pairs.append(("d_modal", ref["d_modal"], ref["b_modal"]))
            if "d_emb" in ref:
                read = ref["emb_cnt"] > 0
                pairs.append(("d_emb", ref["d_emb"][read], ref["b_emb"][read]))
            for k, v, b in pairs:
                over[k] = over.get(k, 0) + int((b.reshape(-1) > v.abs().reshape(-1)).sum())
                total[k] = total.get(k, 0) + v.numel()
    capsys.readouterr()
    with capsys.disabled():
        print("\n[front] share of elements with bound > |reference|, " + str(dtype) + ": "
              + ", ".join(f"{k} {over[k] / total[k]:.2e}" for k in sorted(total)))
    for k in total:
        assert over[k] <= 0.01 * total[k], (k, over[k], total[k])


# ---- refusals that need no device ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from vct_amd import _lib
    return _lib


def _fx(L, dtype, Ts, d, buf, **kw):
    desc = L.EncFrontendExDesc()
    desc.dtype, desc.n, desc.B, desc.d = L.dtype_code(dtype), len(Ts), 1, d
    for i, t in enumerate(Ts):
        desc.T[i] = t
        desc.u[i] = desc.du[i] = buf
    desc.temp = desc.x0 = desc.dx = desc.labels = desc.modal_w = buf
    desc.n_labels = 2 * len(Ts)
    for k, v in kw.items():
        setattr(desc, k, v)
    return desc


def test_refusals_return_the_header_codes(lib):
    """Every call here is refused by the host-side checks in front of any launch: the pointers (one aligned host buffer) are never read."""
    L = lib
    so = L.load()
    hold = ctypes.create_string_buffer(256)
    buf = (ctypes.addressof(hold) + 63) // 64 * 64
    for fn in (so.vct_enc_frontend_ex_fwd, so.vct_enc_frontend_ex_bwd):
        assert fn(ctypes.byref(_fx(L, F32, (3,), 1028, buf)), None) == E_SHAPE
        assert fn(ctypes.byref(_fx(L, BF, (3,), 1032, buf)), None) == E_SHAPE
        assert fn(ctypes.byref(_fx(L, F32, (1024,), 8, buf)), None) == E_SHAPE              # S = 1025
        assert fn(ctypes.byref(_fx(L, F32, (1000, 23), 8, buf)), None) == E_SHAPE           # S = 1025 over two streams
        assert fn(ctypes.byref(_fx(L, F32, (3, 0), 8, buf)), None) == E_SHAPE               # T_i = 0
        assert fn(ctypes.byref(_fx(L, F32, (3, 2), 8, buf, n_labels=3)), None) == E_SHAPE
        assert fn(ctypes.byref(_fx(L, F32, (3,), 8, buf, p_drop=1.0)), None) == E_ARG
    for fn in (so.vct_mm_frontend_fwd, so.vct_mm_frontend_bwd):
        def mm(Ts, n_labels=None):
            desc = L.MmFrontendDesc()
            desc.dtype, desc.n, desc.B, desc.d, desc.n_labels = L.dtype_code(F32), len(Ts), 1, 8, 2 * len(Ts) if n_labels is None else n_labels
            for i, t in enumerate(Ts):
                desc.T[i] = t
                desc.u[i] = desc.du[i] = buf
            desc.temp = desc.modal_w = desc.labels = desc.x0 = desc.dx = desc.d_modal = buf
            return desc
        assert fn(ctypes.byref(mm((3,))), None) == E_SHAPE                                   # n = 1
        assert fn(ctypes.byref(mm((3, 2), 3)), None) == E_SHAPE
        assert fn(ctypes.byref(mm((3, 0))), None) == E_SHAPE
        assert fn(ctypes.byref(mm((1000, 23))), None) == E_SHAPE                             # S = 1025
    hm = L.HmmMixDesc()
    hm.dtype, hm.B, hm.S, hm.d = L.dtype_code(F32), 1, 1025, 8
    hm.take = hm.y = hm.x0 = hm.x = hm.dx = hm.dy = hm.acc = buf
    assert so.vct_hmm_mix_fwd(ctypes.byref(hm), None) == E_SHAPE and so.vct_hmm_mix_bwd(ctypes.byref(hm), None) == E_SHAPE
    hm.S, hm.init, hm.dx0 = 4, 1, buf
    assert so.vct_hmm_mix_bwd(ctypes.byref(hm), None) == E_ARG                               # init together with dx0
    assert so.vct_transpose(L.dtype_code(F32), 8, 8, buf, 8, buf, 8, None) == E_ARG
    for a in (F32, BF):
        for b in (F32, BF):
            assert so.vct_cast(L.dtype_code(a), L.dtype_code(b), buf, buf, 0, None) == E_SHAPE
