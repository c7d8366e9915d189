"""The optimizer's multi-range pass skips token-embedding rows that never had a gradient (vct_adam_step_ranges_rows, the live table
of vct_embed_bwd_live / vct_embed_live_rebuild): a skipped row is one the update would not change, so every check is BITWISE
against the dense pass (vct_adam_step_ranges without a table) -- kernel level on a 300-row table (d = 512: a wave owns whole rows;
d = 96: a row length that does not divide the workgroup's 4096 elements) beside a bias-like range without a table, and trainer
level on the tiny golden model with the switch off and on, eager and as a recorded launch list."""
import numpy as np
import pytest
import torch

import adam_live_ref as R
from helpers import build_model, golden_params, load_golden, model_config_of
import vct_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
V, PAD, ORIGIN, BIAS = 300, 0, 1024, 1000
NEVER = (1, 150, 299)          # rows no batch touches
ONCE, LATE = 7, 200            # touched at step 1 only / first touched at step 3


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from vct_amd import ops as _ops
    return _ops


def bits(t):
    return t.contiguous().view(torch.int32)


def same(a, b):
    return torch.equal(bits(a), bits(b))


_IDS = {}


def batch_ids(step):
    """int64 [4, 8]: pad ids and ids outside [0, V) in every batch (they mark nothing and own no row).  One tensor per step, kept:
    a recorded launch reads it at replay time."""
    if step not in _IDS:
        _IDS[step] = _make_ids(step)
    return _IDS[step]


def _make_ids(step):
    g = torch.Generator().manual_seed(500 + step)
    ids = torch.randint(10, 140, (4, 8), generator=g)
    ids[ids == ONCE] = 8
    ids[:, 0] = 101                                      # [CLS]-like: in every caption
    ids[1, 5:] = PAD
    ids[2, 6], ids[2, 7], ids[3, 7], ids[0, 7] = -3, V, V + 5, 2 ** 31 + 7
    if step == 1:
        ids[0, 3] = ONCE
    if step >= 3:
        ids[3, 2] = LATE
    return ids.to(DEV)


class State:
    """Flat buffers [bias-like range | gap | table V x d | 64 elements of padding], two optimizers' worth of them."""

    def __init__(self, ops, d, hyper=(2e-3, 0.9, 0.999, 1e-8, 0.0)):
        self.ops, self.d = ops, d
        self.n = ORIGIN + V * d + 64
        g = torch.Generator().manual_seed(d)
        self.p = torch.randn(self.n, generator=g).to(DEV)
        self.m = torch.zeros(self.n, device=DEV)
        self.v = torch.zeros(self.n, device=DEV)
        self.m[:BIAS] = (torch.randn(BIAS, generator=g) * 0.01).to(DEV)       # the bias-like range has a history
        self.v[:BIAS] = ((torch.randn(BIAS, generator=g) * 0.01) ** 2).to(DEV)
        self.g = torch.zeros(self.n, device=DEV)
        self.gbias = (torch.randn(4, self.n, generator=g) * 0.01).to(DEV)      # per step: gradients of the bias range and the padding
        self.shadow = torch.zeros(self.n, dtype=torch.bfloat16, device=DEV)
        self.step = torch.zeros(1, dtype=torch.int32, device=DEV)
        self.hyper = torch.tensor(list(hyper) + [0, 0, 0], dtype=torch.float32, device=DEV)
        self.live = torch.zeros(V, dtype=torch.uint8, device=DEV)
        self.ws = torch.zeros(2 * V + 4 + 64, dtype=torch.int32, device=DEV)
        self.dx = torch.randn(32, d, generator=g).to(DEV)
        self.ranges = [(0, BIAS, True), (ORIGIN, self.n, False)]
        self.dense = ops.adam_ranges_table(self.ranges, DEV)
        self.rows = ops.adam_ranges_table(self.ranges, DEV, {1: (ORIGIN, d, V, self.live)})
        assert len(self.dense) == 3 and len(self.rows) == 5

    def table(self, t):
        return t[ORIGIN:ORIGIN + V * self.d].view(V, self.d)

    def clone(self):
        c = object.__new__(State)
        c.__dict__.update(self.__dict__)
        for k in ("p", "m", "v", "g", "shadow", "step", "live", "ws"):
            setattr(c, k, getattr(self, k).clone())
        c.rows = self.ops.adam_ranges_table(self.ranges, DEV, {1: (ORIGIN, self.d, V, c.live)})
        return c

    def backward(self, k, mark):
        """Step k's gradients: the embedding scatter (which marks the live table when asked to) and the rest."""
        self.ops.embed_bwd(batch_ids(k), 8, PAD, self.dx, self.table(self.g), id_ws=self.ws, live=self.live if mark else None)
        self.g[:BIAS] = self.gbias[k - 1, :BIAS]
        self.g[self.n - 64:] = self.gbias[k - 1, self.n - 64:]

    def adam(self, rows):
        self.ops.adam_step_ranges(self.p, self.g, self.m, self.v, self.shadow, self.rows if rows else self.dense, 0, 0, 0, 0, 0,
                                  self.step, hyper=self.hyper)
        self.ops.adam_bump(self.step)

    def snap(self):
        torch.cuda.synchronize()
        return tuple(t.clone() for t in (self.p, self.m, self.v, self.shadow))


@pytest.fixture(scope="module", params=[512, 96])
def four_steps(ops, request):
    """4 consecutive steps, dense and row-aware, from the same start: (d, start, [dense snapshots], [row-aware snapshots], live
    table after each step)."""
    s0 = State(ops, request.param)
    a, b = s0.clone(), s0.clone()
    start = s0.snap()
    da, db, lives = [], [], []
    for k in range(1, 5):
        a.backward(k, mark=False); a.adam(rows=False); da.append(a.snap())
        b.backward(k, mark=True); b.adam(rows=True); db.append(b.snap())
        lives.append(b.live.cpu().numpy().copy())
    assert int(a.step) == 4 and int(b.step) == 4
    assert not bool(a.live.any())                        # the dense twin never marked anything
    return request.param, start, da, db, lives


def test_every_step_is_bitwise_the_dense_pass(four_steps):
    d, start, da, db, _ = four_steps
    for k in range(4):
        for x, y in zip(da[k], db[k]):
            assert same(x, y), (d, k)
    # ... and something happened: the bias-like range, the padding behind the table and the touched rows moved
    assert not same(db[0][0][:BIAS], start[0][:BIAS]) and not same(db[0][0][-64:], start[0][-64:])
    assert not same(db[0][3][:BIAS], start[3][:BIAS])                         # its bf16 shadow was written


def test_rows_never_touched_keep_their_initial_bits(four_steps):
    d, start, da, db, lives = four_steps
    for r in NEVER:
        sl = slice(ORIGIN + r * d, ORIGIN + (r + 1) * d)
        for k in range(4):
            for i in range(3):
                assert same(db[k][i][sl], start[i][sl]) and same(da[k][i][sl], start[i][sl]), (d, r, k, i)
        assert lives[3][r] == 0


def test_a_row_first_touched_at_step_three_follows_the_dense_pass_from_then_on(four_steps):
    d, start, da, db, lives = four_steps
    sl = slice(ORIGIN + LATE * d, ORIGIN + (LATE + 1) * d)
    assert lives[0][LATE] == 0 and lives[1][LATE] == 0 and lives[2][LATE] == 1 and lives[3][LATE] == 1
    for k in (0, 1):
        assert same(db[k][0][sl], start[0][sl]) and same(db[k][1][sl], start[1][sl])
    for k in (2, 3):
        for i in range(3):
            assert same(db[k][i][sl], da[k][i][sl])
        assert not same(db[k][0][sl], db[k - 1][0][sl])


def test_a_row_touched_once_keeps_being_stepped(four_steps):
    """Its gradient is zero from step 2 on, its moments are not: they decay and move the parameter."""
    d, start, da, db, lives = four_steps
    sl = slice(ORIGIN + ONCE * d, ORIGIN + (ONCE + 1) * d)
    assert all(lv[ONCE] == 1 for lv in lives)
    for k in range(1, 4):
        for i in range(3):
            assert same(db[k][i][sl], da[k][i][sl])
            assert not same(db[k][i][sl], db[k - 1][i][sl]), (d, k, i)


def test_marks_are_exactly_the_ids_inside_the_table_that_are_not_padding(four_steps):
    d, _, _, _, lives = four_steps
    want = np.zeros(V, np.uint8)
    for k in range(1, 5):
        want |= R.marked_rows(batch_ids(k).cpu().numpy(), PAD, V)
        assert np.array_equal(lives[k - 1], want), (d, k)
    assert want[PAD] == 0 and want[101] == 1 and 20 < int(want.sum()) < 140


@pytest.mark.parametrize("d", [512, 96])
@pytest.mark.parametrize("hyper", [(2e-3, 0.9, 0.999, 1e-8, 0.01), (2e-3, 0.9, 0.999, 0.0, 0.0)], ids=["weight_decay", "eps0"])
def test_no_skip_when_a_zero_row_is_not_a_fixed_point(ops, d, hyper):
    """Weight decay moves every parameter and eps = 0 turns 0 / 0 into NaN: with a live table that marks NOTHING the row-aware
    launch must still give the dense result -- the kernel reads the hyper-parameters from the device block and does not skip."""
    assert not R.zero_row_is_noop(*hyper, 1) and R.zero_row_is_noop(2e-3, 0.9, 0.999, 1e-8, 0.0, 1)
    s0 = State(ops, d, hyper)
    a, b = s0.clone(), s0.clone()
    start = s0.snap()
    for k in (1, 2):
        a.backward(k, mark=False); a.adam(rows=False)
        b.backward(k, mark=False); b.adam(rows=True)
    assert not bool(b.live.any())
    for x, y in zip(a.snap(), b.snap()):
        assert same(x, y)
    r = NEVER[0]
    assert not same(b.p[ORIGIN + r * d:ORIGIN + (r + 1) * d], start[0][ORIGIN + r * d:ORIGIN + (r + 1) * d])


@pytest.mark.parametrize("d", [512, 96])
def test_rebuild_finds_rows_with_moments(ops, d):
    """Moments written from outside (a loaded optimizer state) into rows no batch marked: vct_embed_live_rebuild makes them live
    and they are stepped like the dense pass steps them.  -0.0 counts (the update turns it into +0.0)."""
    s0 = State(ops, d)
    s0.table(s0.m)[250, 3] = 0.25
    s0.table(s0.v)[251, d - 1] = 1e-4
    s0.table(s0.m)[252, 0] = -0.0
    a, b = s0.clone(), s0.clone()
    b.backward(1, mark=True)
    marked = b.live.cpu().numpy().copy()
    ops.embed_live_rebuild(b.live, b.table(b.m), b.table(b.v), b.table(b.g))
    torch.cuda.synchronize()
    want = R.live_from_buffers(b.table(b.m).cpu().numpy(), b.table(b.v).cpu().numpy(), b.table(b.g).cpu().numpy())
    assert np.array_equal(b.live.cpu().numpy(), want)
    assert all(want[r] == 1 and marked[r] == 0 for r in (250, 251, 252)) and want[NEVER[0]] == 0
    assert np.array_equal(want | marked, want)           # every marked row has a gradient here (dx has no zero row)
    a.backward(1, mark=False)
    a.adam(rows=False); b.adam(rows=True)
    for x, y in zip(a.snap(), b.snap()):
        assert same(x, y)
    assert not same(b.table(b.p)[250], s0.table(s0.p)[250])
    assert bits(b.table(b.m)[252, :1]).item() == 0       # -0.0 became +0.0, as in the dense pass


@pytest.mark.parametrize("d", [512, 96])
def test_replayed_launch_list_equals_eager_steps(ops, d):
    """[embedding backward that marks, row-aware pass, counter bump] recorded once and replayed twice == two eager steps: the live
    table is device memory the recorded launches write and read."""
    s0 = State(ops, d)
    a, b = s0.clone(), s0.clone()
    for _ in range(2):
        a.backward(3, mark=True); a.adam(rows=True)
    ll = ops.LaunchList()
    with ll.record():
        b.backward(3, mark=True); b.adam(rows=True)
    torch.cuda.synchronize()
    assert not bool(b.live.any()) and int(b.step) == 0    # recording executed nothing
    ll.replay(); ll.replay()
    for x, y in zip(a.snap(), b.snap()):
        assert same(x, y)
    assert int(b.step) == 2 and np.array_equal(b.live.cpu().numpy(), R.marked_rows(batch_ids(3).cpu().numpy(), PAD, V))
    assert torch.equal(a.live, b.live)
    c = s0.clone()                                        # ... and both are the dense result
    for _ in range(2):
        c.backward(3, mark=False); c.adam(rows=False)
    for x, y in zip(c.snap(), b.snap()):
        assert same(x, y)


# ---- trainer level: the tiny golden model, switch off / on, eager / recorded ---------------------------------------------------------

def _tiny():
    z = load_golden("tiny_train.npz")
    mc = model_config_of(z)
    cfg = O.cfg_from_model_config(mc, int(z["vocab"]))
    return z, mc, golden_params(z, cfg)


def _train(monkeypatch, live, executor, round_trip=False):
    from vct_amd.trainer import CaptionTrainer, FusedAdam
    monkeypatch.setattr(FusedAdam, "live_rows", bool(live))
    z, mc, p = _tiny()
    torch.manual_seed(7)                                  # the parameters the golden file does not carry (matching.*) are drawn
    m = build_model(mc, int(z["vocab"]), DEV, torch.bfloat16, p)
    m.train()
    opt = FusedAdam(m, lr=1e-3)
    tr = CaptionTrainer(m, opt, launch_list=executor == "list")
    assert tr.fuse_adam
    feats, mask = torch.from_numpy(z["feats"]).to(DEV), torch.from_numpy(z["mask"]).to(DEV)
    ids = torch.from_numpy(z["ids"]).to(DEV)
    losses = []
    for k in range(4):
        if round_trip and k == 2:                         # a checkpoint resume in the middle: the table is rebuilt from the moments
            sd = opt.state_dict()
            opt.exp_avg.zero_(); opt.exp_avg_sq.zero_()
            opt.load_state_dict(sd)
        losses.append(tr.step(feats, mask, torch.roll(ids, k, 0) if k % 2 else ids).clone())
    torch.cuda.synchronize()
    used = None if opt._live is None else int(opt._live.sum())
    assert any(k[1] for k in opt._range_tables) == bool(live)      # the row-aware launch is what ran (or never ran)
    return torch.cat(losses), m.flat_params.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), used, int(z["vocab"])


@pytest.fixture(scope="module")
def dense_run():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    mp = pytest.MonkeyPatch()
    try:
        return _train(mp, live=False, executor="eager")
    finally:
        mp.undo()


@pytest.mark.parametrize("round_trip", [False, True], ids=["straight", "state_dict_round_trip"])
@pytest.mark.parametrize("executor", ["eager", "list"])
@pytest.mark.parametrize("live", [False, True], ids=["VCT_ADAM_LIVE=0", "VCT_ADAM_LIVE=1"])
def test_trainer_switch_changes_no_bit(monkeypatch, dense_run, live, executor, round_trip):
    """Four steps: every parameter, both moment buffers and the losses equal the dense eager run bitwise, whichever the switch and
    the executor, with and without a FusedAdam.state_dict() -> load_state_dict() round trip in the middle."""
    l0, p0, m0, v0, used0, vocab = dense_run
    l1, p1, m1, v1, used, _ = _train(monkeypatch, live, executor, round_trip)
    assert same(l0, l1) and same(p0, p1) and same(m0, m1) and same(v0, v1)
    assert used0 is None
    if live:
        assert 0 < used < vocab // 4                      # the batch's distinct non-padding ids, a fraction of the 131 rows
    else:
        assert used is None
