"""CPU checks of tests/row_ref.py, the fp64 references, bounds and checkers of tests/test_row_kernels_gpu.py (no GPU, no library):
  * ln_fwd / ln_bwd against torch.nn.functional.layer_norm and autograd, adam against torch.optim.Adam / AdamW over three steps, sce
    against oracle/vct_oracle.py (sce_loss), the embedding against index_add_, all in fp64;
  * a CORRECT float32 emulation of every operation stays inside the derived bounds at every entry of row_ref.SHAPES (the worst
    |delta| / bound is printed per operation and must be below 1);
  * every fault of row_ref.FAULTS is rejected by the checker the GPU file uses for it, on at least one listed shape -- the evidence that
    the GPU tests would fail on a subtly wrong kernel;
  * the share of loss elements beside the p = 1e-7 clamp is at most 1 % in every loss case, and every alpha != 1 case has a row with
    columns below the clamp and a row whose label column is below it (V = 1 has one column with p = 1: no such row exists)."""
import pytest
import torch

import row_ref as R
import vct_oracle as O

F64, F32, BF = R.F64, R.F32, R.BF
S = R.SHAPES
DROP = (1234, 5, 0.3)


def _mask(M, d, p):
    return R.drop_mask(M, d, DROP) if p > 0 else None


# ---- the references against torch / the oracle -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_res", [True, False])
def test_ln_reference_is_layer_norm_and_autograd(with_res):
    M, d = 7, 36
    x = R.rnd((M, d), 1).double().requires_grad_(True)
    res = R.rnd((M, d), 2).double().requires_grad_(True) if with_res else None
    g, b = (t.double().requires_grad_(True) for t in R.ln_params(d, 3))
    mask = R.drop_mask(M, d, DROP)
    s = x * mask + res if with_res else x * mask
    s.retain_grad()
    y = torch.nn.functional.layer_norm(s, (d,), g, b, 1e-5)
    dy = R.rnd((M, d), 4).double()
    y.backward(dy)
    f = R.ln_fwd(x.detach(), None if res is None else res.detach(), g.detach(), b.detach(), mask)
    assert torch.allclose(f["y"], y.detach(), rtol=1e-12, atol=1e-13)
    assert torch.allclose(f["mean"], s.detach().mean(1), rtol=1e-13)
    assert torch.allclose(f["rstd"], 1 / torch.sqrt(s.detach().var(1, unbiased=False) + 1e-5), rtol=1e-13)
    r = R.ln_bwd(dy, x.detach(), None if res is None else res.detach(), g.detach(), f["mean"], f["rstd"], mask)
    assert torch.allclose(r["ds"], s.grad, rtol=1e-10, atol=1e-13)
    assert torch.allclose(r["dxo"], x.grad, rtol=1e-10, atol=1e-13)
    assert torch.allclose(r["dgamma"], g.grad, rtol=1e-10, atol=1e-13) and torch.allclose(r["dbeta"], b.grad, rtol=1e-12)
    # two norms: the front norm's ds (its gradient of y) is the dy of the layer norm
    g2, b2 = (t.double() for t in R.ln_params(d, 9))
    x2 = x.detach().clone().requires_grad_(True)
    y1 = torch.nn.functional.layer_norm(x2, (d,), g.detach(), b.detach(), 1e-5)
    y1.retain_grad()
    torch.nn.functional.layer_norm(y1, (d,), g2, b2, 1e-5).backward(dy)
    f2 = R.ln_fwd(y1.detach(), None, g2, b2)
    front = R.ln_bwd(dy, y1.detach(), None, g2, f2["mean"], f2["rstd"])
    assert torch.allclose(front["ds"], y1.grad, rtol=1e-10, atol=1e-13)
    f1 = R.ln_fwd(x.detach(), None, g.detach(), b.detach())
    assert torch.allclose(R.ln_bwd(front["ds"], x.detach(), None, g.detach(), f1["mean"], f1["rstd"])["ds"], x2.grad, rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("wd", S["adam_wd"])
def test_adam_reference_is_torch_optim_over_three_steps(wd):
    hp = [R.f32v(z) for z in (1e-3, 0.9, 0.999, 1e-8, wd)]
    p0 = R.adam_case(64, 3)[0]
    w = torch.nn.Parameter(p0.double().clone())
    opt = (torch.optim.AdamW if wd else torch.optim.Adam)([w], lr=hp[0], betas=(hp[1], hp[2]), eps=hp[3], weight_decay=hp[4])
    p, m, v = p0.double(), torch.zeros(64, dtype=F64), torch.zeros(64, dtype=F64)
    for step in range(3):
        g = R.rnd((64,), 20 + step, 1e-2).double()
        w.grad = g.clone()
        opt.step()
        r = R.adam(p, g, m, v, *hp, step)
        p, m, v = r["p"], r["m"], r["v"]
        assert torch.allclose(p, w.detach(), rtol=1e-12, atol=1e-15), step
    st = opt.state[w]
    assert torch.allclose(m, st["exp_avg"], rtol=1e-12, atol=1e-300) and torch.allclose(v, st["exp_avg_sq"], rtol=1e-12, atol=1e-300)


@pytest.mark.parametrize("alpha", S["sce_alpha"])
def test_sce_reference_is_the_oracle(alpha):
    """Without pads (every row counts; the pad rows of the case get label 0), at the small vocabularies too."""
    for V in (1, 3, 5, 257):
        x, ids, pad = R.sce_case(V, 11, F32)
        lab = ids[:, 1:].reshape(-1)
        lab = torch.where(lab == pad, torch.zeros_like(lab), lab)
        r = R.sce(x, lab, alpha, -7)
        loss, grad = O.sce_loss(x.double().numpy(), lab.numpy(), alpha, pad_id=-7)
        assert abs(float(r["loss"]) - float(loss)) <= 1e-12 * abs(float(loss)), V
        assert torch.allclose(r["grad"], torch.from_numpy(grad), rtol=1e-11, atol=1e-15), V


def test_sce_reference_with_pads_is_the_oracle():
    """Pad rows keep their own label column (the pad id, inside the vocabulary) in kernel and oracle alike."""
    for alpha in S["sce_alpha"]:
        for V in (4, 9, 257):
            x, ids, pad = R.sce_case(V, 12, F32)
            lab = ids[:, 1:].reshape(-1)
            assert pad == 1 and int((lab == pad).sum()) == 3
            r = R.sce(x, lab, alpha, pad)
            loss, grad = O.sce_loss(x.double().numpy(), lab.numpy(), alpha, pad_id=pad)
            assert abs(float(r["loss"]) - float(loss)) <= 1e-12 * abs(float(loss)), (alpha, V)
            assert torch.allclose(r["grad"], torch.from_numpy(grad), rtol=1e-11, atol=1e-15), (alpha, V)


def test_embedding_reference_is_gather_and_index_add():
    ids, Sq, V, pad = R.embed_ids("mixed")
    flat = ids[:, :Sq].reshape(-1)
    d = 8
    dx = R.rnd((flat.numel(), d), 5).double()
    out, e, cnt = R.embed_bwd(flat, dx, V, pad)
    ok = (flat != pad) & (flat >= 0) & (flat < V)
    ref = torch.zeros(V, d, dtype=F64).index_add_(0, flat[ok], dx[ok])
    assert torch.equal(out, ref) and float(out[pad].abs().sum()) == 0.0
    assert [int(cnt[i]) for i in (5, 6, 7, 8)] == [40, 9, 8, 1] and int((cnt == 1).sum()) > 200
    table, pos = R.rnd((V, d), 6), R.rnd((Sq, d), 7)
    good = torch.where(ok, flat, torch.zeros_like(flat))
    x, _ = R.embed_fwd(good, table, pos, Sq)
    assert torch.equal(x, (table.double()[good].view(-1, Sq, d) + pos.double()[None]).view(-1, d))
    for kind, n in (("same", 1100), ("far", 1092)):
        ids, Sq, V, pad = R.embed_ids(kind)
        assert int((ids[:, :Sq] == 3).sum()) == n


# ---- the clean emulation inside the bounds, at every shape -----------------------------------------------------------------------------------
def _ln_inputs(M, d, dtype, p, with_res, seed):
    x, res = R.ln_rows(M, d, seed, dtype, with_res)
    gamma, beta = R.ln_params(d, seed + 5)
    dy = R.rnd((M, d), seed + 7, 1.0, dtype)
    return x, res, gamma, beta, dy, _mask(M, d, p)


def _run(failed, name, fn, *args, **kw):
    """One checker.  failed = None: it raises as in the GPU file.  failed = a list: a rejection is recorded under the checker's name
    (so a fault test can require the rejection of the checker MEANT for the fault, not of any), and every checker still runs."""
    if failed is None:
        return fn(*args, **kw) or 0.0
    try:
        return fn(*args, **kw) or 0.0
    except AssertionError:
        failed.append(name)
        return 0.0


# the checker(s) each fault must be rejected by
MEANT = {
    "mean_drops_last_vector": {"mean"}, "one_pass_variance": {"rstd"}, "rstd_without_eps": {"rstd"}, "neighbour_row_statistic": {"mean"},
    "truncate_bf16": {"y"}, "dgamma_misses_last_partial": {"dgamma"}, "dgamma_dbeta_swapped": {"dgamma", "dbeta"},
    "dxo_not_masked": {"dxo", "dxo mask"}, "padding_counted_small": {"RCE rows"}, "label_left_in_q": {"RCE rows"},
    "nvalid_counts_pads": {"gradient"}, "gradient_small_branch_everywhere": {"gradient"}, "t_is_step": {"p"}, "decay_after_step": {"p"},
    "drop_one_occurrence": {"dtable"},
}


def _check_ln(tag, dtype, x, res, gamma, beta, dy, mask, fwd_fault=None, bwd_fault=None, failed=None):
    f = R.ln_fwd(x, res, gamma, beta, mask)
    y, mean, rstd = R.emulate("ln_fwd", x, res, gamma, beta, mask, dtype, fault=fwd_fault)
    worst = [_run(failed, "y", R.check_elem, f"{tag} y", y, f["y"], R.bound(f["y"], f["e_y"], dtype)),
             _run(failed, "mean", R.check_elem, f"{tag} mean", mean, f["mean"], R.bound(f["mean"], f["e_mean"], F32)),
             _run(failed, "rstd", R.check_elem, f"{tag} rstd", rstd, f["rstd"], R.bound(f["rstd"], f["e_rstd"], F32))]
    mean32, rstd32 = f["mean"].to(F32), f["rstd"].to(F32)
    b = R.ln_bwd(dy, x, res, gamma, mean32, rstd32, mask)
    ds, dxo, dg, db = R.emulate("ln_bwd", dy, x, res, gamma, mean32, rstd32, mask, dtype, fault=bwd_fault)
    worst += [_run(failed, "ds", R.check_elem, f"{tag} ds", ds, b["ds"], R.bound(b["ds"], b["e_ds"], dtype)),
              _run(failed, "dxo", R.check_elem, f"{tag} dxo", dxo, b["dxo"], R.bound(b["dxo"], b["e_dxo"], dtype)),
              _run(failed, "dgamma", R.check_elem, f"{tag} dgamma", dg, b["dgamma"], R.bound(b["dgamma"], b["e_dgamma"], F32)),
              _run(failed, "dbeta", R.check_elem, f"{tag} dbeta", db, b["dbeta"], R.bound(b["dbeta"], b["e_dbeta"], F32))]
    if mask is not None:
        _run(failed, "dxo mask", R.check_mask, f"{tag} dxo mask", dxo, b["dxo"], R.bound(b["dxo"], b["e_dxo"], dtype))
    return max(worst)


@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
def test_layernorm_emulation_stays_inside_the_bounds(dtype, capsys):
    worst = 0.0
    for d in S["ln_d"][dtype]:
        for M in S["ln_M"]:
            for i, (p, with_res) in enumerate(S["ln_modes"]):
                worst = max(worst, _check_ln(f"ln {M}x{d} p={p} res={with_res}", dtype, *_ln_inputs(M, d, dtype, p, with_res, 100 + d + M + i)))
    capsys.readouterr()
    with capsys.disabled():
        print(f"\n[row] layernorm {dtype}: clean emulation, worst |delta| / bound = {worst:.3f}")
    assert worst < 1.0


LN_FAULT_SHAPES = ((5, 8), (37, 8), (37, 256), (5, 520))


@pytest.mark.parametrize("fault", [f for f, op in R.FAULTS.items() if op in ("ln_fwd", "ln_bwd")])
def test_layernorm_checkers_reject_the_seeded_faults(fault, capsys):
    hits = []
    for dtype in ((BF,) if fault == "truncate_bf16" else (F32, BF)):
        for (M, d) in LN_FAULT_SHAPES:
            for (p, with_res) in ((0.3, True), (0.0, False)):
                args = _ln_inputs(M, d, dtype, p, with_res, 300 + d + M)
                kw = {"fwd_fault": fault} if R.FAULTS[fault] == "ln_fwd" else {"bwd_fault": fault}
                failed = []
                _check_ln(f"{fault} {M}x{d}", dtype, *args, failed=failed, **kw)
                if MEANT[fault] <= set(failed):
                    hits.append((dtype, M, d, p, with_res))
    capsys.readouterr()
    with capsys.disabled():
        print(f"\n[row] fault {fault}: rejected by {sorted(MEANT[fault])} on {len(hits)} of the cases tried, first {hits[:1]}")
    assert hits, fault


def _sce_cases(dtype):
    for V in S["sce_V"][dtype]:
        for alpha in S["sce_alpha"]:
            yield V, alpha


def _check_sce(tag, dtype, V, alpha, seed=40, fault=None, tile=None, failed=None):
    x, ids, pad = R.sce_case(V, seed, dtype)
    lab = ids[:, 1:].reshape(-1)
    r = R.sce(x, lab, alpha, pad, dtype)
    loss, grad, ce, rce = R.emulate("sce", x, lab, alpha, pad, dtype, tile, fault=fault)
    w = [_run(failed, "gradient", R.check_elem, f"{tag} gradient", grad, r["grad"], r["b_grad"], alt=r["alt"]),
         _run(failed, "CE rows", R.check_elem, f"{tag} CE rows", ce, r["ce_rows"], r["b_ce"]),
         _run(failed, "loss", R.check_elem, f"{tag} loss", loss.reshape(1), r["loss"].reshape(1), r["b_loss"].reshape(1))]
    if alpha != 1.0:
        w.append(_run(failed, "RCE rows", R.check_elem, f"{tag} RCE rows", rce, r["rce_rows"], r["b_rce"]))
    return max(w), r


@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
def test_sce_emulation_stays_inside_the_bounds_and_the_cases_hold_what_they_must(dtype, capsys):
    worst = 0.0
    for V, alpha in _sce_cases(dtype):
        w, r = _check_sce(f"sce V={V} alpha={alpha}", dtype, V, alpha)
        worst = max(worst, w)
        assert torch.equal(r["alt"][~r["near"]], r["grad"][~r["near"]]), "the other branch is accepted beside the clamp only"
        share = float(r["near"].double().mean())
        assert share <= 0.01, (V, alpha, share)
        if alpha != 1.0 and V > 1:
            assert bool(r["small"][0].any()), "row 0 has columns below the clamp"
            assert float(r["py"][1]) < R.CLAMP, "row 1's label column is below the clamp"
        assert int(r["y"][0]) == 0 and int(r["y"][1]) == V - 1 and int(r["nvalid"]) == 3
    capsys.readouterr()
    with capsys.disabled():
        print(f"\n[row] sce {dtype}: clean emulation, worst |delta| / bound = {worst:.3f}")
    assert worst < 1.0


@pytest.mark.parametrize("fault", [f for f, op in R.FAULTS.items() if op == "sce"])
def test_sce_checkers_reject_the_seeded_faults(fault, capsys):
    hits = []
    for dtype in (F32, BF):
        for V in (7 if dtype == BF else 5, 257):
            for alpha in (0.5, 0.0) if fault != "nvalid_counts_pads" else (1.0, 0.5):
                failed = []
                _check_sce(f"{fault} V={V}", dtype, V, alpha, fault=fault, failed=failed)
                if MEANT[fault] <= set(failed):
                    hits.append((dtype, V, alpha))
    capsys.readouterr()
    with capsys.disabled():
        print(f"\n[row] fault {fault}: rejected by {sorted(MEANT[fault])} on {len(hits)} of 8 cases, first {hits[:1]}")
    assert hits, fault


HP = (1e-3, 0.9, 0.999, 1e-8)


def _check_adam(tag, n, step, wd, fault=None, failed=None):
    p, g, m, v = R.adam_case(n, 50 + step)
    r = R.adam(p, g, m, v, *HP, wd, step)
    p2, m2, v2, sh = R.emulate("adam", p, g, m, v, *HP, wd, step, fault=fault)
    assert torch.equal(sh, p2.to(BF))
    return max(_run(failed, "p", R.check_elem, f"{tag} p", p2, r["p"], R.bound(r["p"], r["e_p"], F32)),
               _run(failed, "m", R.check_elem, f"{tag} m", m2, r["m"], R.bound(r["m"], r["e_m"], F32)),
               _run(failed, "v", R.check_elem, f"{tag} v", v2, r["v"], R.bound(r["v"], r["e_v"], F32)))


def test_adam_emulation_stays_inside_the_bounds(capsys):
    worst = 0.0
    for n in S["adam_n"]:
        for step in S["adam_step"]:
            for wd in S["adam_wd"]:
                worst = max(worst, _check_adam(f"adam n={n} step={step} wd={wd}", min(n, 1028), step, wd))     # elements are independent
    capsys.readouterr()
    with capsys.disabled():
        print(f"\n[row] adam: clean emulation, worst |delta| / bound = {worst:.3f}")
    assert worst < 1.0


@pytest.mark.parametrize("fault", [f for f, op in R.FAULTS.items() if op == "adam"])
def test_adam_checker_rejects_the_seeded_faults(fault, capsys):
    hits = []
    for step in (1, 999):
        failed = []
        _check_adam(f"{fault} step={step}", 1024, step, 0.01, fault=fault, failed=failed)
        if MEANT[fault] <= set(failed):
            hits.append(step)
    capsys.readouterr()
    with capsys.disabled():
        print(f"\n[row] fault {fault}: rejected by {sorted(MEANT[fault])} at steps {hits}")
    assert hits, fault


def _check_embed(tag, kind, d, dtype, p, exact, fault=None):
    ids, Sq, V, pad = R.embed_ids(kind)
    flat = ids[:, :Sq].reshape(-1)
    N = flat.numel()
    mask = R.drop_mask(N, d, DROP) if p > 0 else None
    dx = (R.G.ints((N, d), 70, dtype) if exact else R.rnd((N, d), 71, 1.0, dtype))
    ref, e, _ = R.embed_bwd(flat, dx, V, pad, mask)
    got = R.emulate("embed_bwd", flat, dx, V, pad, mask, fault=fault)
    if exact:
        R.check_exact(f"{tag} dtable", got, ref)
        return 0.0
    return R.check_elem(f"{tag} dtable", got, ref, R.bound(ref, e, F32))


def test_embedding_emulation_stays_inside_the_bounds(capsys):
    worst = 0.0
    for kind in S["emb_kinds"]:
        for d in (4, 8, 64) if kind == "mixed" else (8,):              # (columns are independent: the wide tables add nothing on the CPU)
            for dtype in (F32, BF) if d % 8 == 0 else (F32,):
                worst = max(worst, _check_embed(f"embed {kind} d={d}", kind, d, dtype, 0.3, False))
                _check_embed(f"embed {kind} d={d} ints", kind, d, dtype, 0.0, True)
    ids, Sq, V, pad = R.embed_ids("mixed")
    good = torch.where((ids >= 0) & (ids < V), ids, torch.zeros_like(ids))[:, :Sq].reshape(-1)
    for dtype in (F32, BF):
        table, pos = R.rnd((V, 8), 6), R.rnd((Sq, 8), 7)
        mask = R.drop_mask(good.numel(), 8, DROP)
        x, e = R.embed_fwd(good, table, pos, Sq, mask)
        got = R.emulate("embed_fwd", good, table, pos, Sq, mask, dtype)
        worst = max(worst, R.check_elem("embed fwd", got, x, R.bound(x, e, dtype)))
        R.check_mask("embed fwd mask", got, x, R.bound(x, e, dtype))
    capsys.readouterr()
    with capsys.disabled():
        print(f"\n[row] embedding: clean emulation, worst |delta| / bound = {worst:.3f}")
    assert worst < 1.0


def test_embedding_checkers_reject_a_dropped_occurrence(capsys):
    hits = 0
    for exact in (True, False):
        with pytest.raises(AssertionError):
            _check_embed("drop_one_occurrence", "mixed", 8, F32, 0.0, exact, fault="drop_one_occurrence")
        hits += 1
    capsys.readouterr()
    with capsys.disabled():
        print(f"\n[row] fault drop_one_occurrence: rejected by the exact check and by the bound check ({hits} of 2)")


def test_mask_checker_rejects_another_mask():
    a, b = R.drop_mask(37, 8, DROP), R.drop_mask(37, 8, (1235, 5, 0.3))
    R.check_mask("same", a, a)
    with pytest.raises(AssertionError):
        R.check_mask("other seed", b, a)
    with pytest.raises(AssertionError):
        R.check_mask("shifted", torch.roll(a, 1, dims=1), a)


def test_every_fault_has_a_rejection_test():
    assert len(R.FAULTS) == 15 and set(MEANT) == set(R.FAULTS) and set(R.FAULTS.values()) == {"ln_fwd", "ln_bwd", "sce", "adam", "embed_bwd"}
