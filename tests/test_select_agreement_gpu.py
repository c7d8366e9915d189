"""The greedy, sampled (top_k = 1) and beam (K = 1) selectors are one rule (csrc/vct_select_core.h): on the same rows each returns
numpy.argmax of the dtype-rounded row, i.e. the FIRST maximal index, wherever the two copies of a row's maximum lie relative to
a thread's 16-byte vector, the waves of a chunk and the chunks of a row."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD, NO_END = 0, -1                                       # no token equals NO_END: nothing ends, nothing finishes
TOP = 12.0                                                # above every other logit (those are < 10)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@functools.lru_cache(maxsize=None)
def _rows(V, dtype):
    """Four rows of logits on a 1/8 grid (exact in bf16) with the row maximum planted twice, and the expected tokens.
    A chunk is 256 threads x 16 bytes: 2048 bf16 or 1024 fp32 columns, a wave's share of it 512 or 256 columns.
      row 0  both copies inside one thread's 16-byte vector (columns 162, 163: one vector of 8 bf16 and of 4 fp32)
      row 1  copies in two different waves of chunk 0 (V = 257 has one wave's worth of bf16 columns: two threads of it)
      row 2  the same offset of chunk 0 and of the last full chunk (one full chunk only: chunk 0 and the tail chunk's lone
             element; V = 257 is a single chunk: two threads of one wave) -- the later copy must never win
      row 3  the only maximum is the last column, V - 1 (for V = 2049 / 4097 the lone element of the tail chunk)."""
    chunk = 256 * (8 if dtype == torch.bfloat16 else 4)
    rng = np.random.default_rng(V)
    x = (rng.integers(-80, 80, (4, V)) / 8.0).astype(np.float32)
    full = V // chunk
    pairs = [(162, 163),
             (40, 640) if V > 1024 else (5, 256),
             (77, (full - 1) * chunk + 77) if full >= 2 else ((77, V - 1) if V > chunk else (77, 200))]
    for r, (a, b) in enumerate(pairs):
        assert 0 <= a < b < V
        x[r, a] = x[r, b] = TOP
    x[3, V - 1] = TOP
    want = np.array([a for a, _ in pairs] + [V - 1])
    xq = torch.from_numpy(x).to(dtype).float().numpy()
    assert np.array_equal(xq, x) and np.array_equal(xq.argmax(1), want)
    return x, want


def _sample_ctl(seed, top_k, temperature, top_p):
    c = np.zeros(1, dtype=[("seed", "<u4"), ("k", "<i4"), ("it", "<f4"), ("p", "<f4")])
    c["seed"], c["k"], c["it"], c["p"] = seed, top_k, np.float32(1.0 / temperature), np.float32(top_p)
    return torch.from_numpy(c.view(np.int32).copy()).to(DEV)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("V", [257, 2049, 4097])
def test_selectors_agree_on_the_first_maximum(V, dtype):
    from vct_amd import ops
    x, want = _rows(V, dtype)
    rows, t, Lmax = x.shape[0], 5, 8
    for ldx in (V + 3, (V + 31) // 32 * 32 + 32):         # odd rows (element loads) and 16-byte rows (vector loads), both > V
        xs = torch.zeros(rows, ldx, dtype=dtype, device=DEV)
        xs[:, :V] = torch.from_numpy(x).to(DEV, dtype)
        xs[:, V:] = 1e4                                   # columns past V must never be read as candidates
        got = {}

        def state():
            return (torch.full((rows, Lmax), -5, dtype=torch.long, device=DEV), torch.zeros(rows, dtype=torch.uint8, device=DEV),
                    torch.zeros(1, dtype=torch.int32, device=DEV), torch.full((1,), Lmax, dtype=torch.long, device=DEV))

        ys, en, cnt, at = state()
        ops.greedy_select(xs, ys[:, t], NO_END, en, cnt, at, t, cols=V)
        got["greedy_select"] = ys[:, t]
        out = torch.full((rows,), -5, dtype=torch.long, device=DEV)
        ops.argmax_rows(xs, out, cols=V)
        got["argmax_rows"] = out
        ws = torch.full((ops.sample_select_workspace_bytes(dtype, rows, V) // 4,), float("nan"), dtype=torch.float32, device=DEV)
        for seed, temperature in ((0, 1.0), (12345, 2.0), (7, 2.0), (4242, 1.0)):
            ys, en, cnt, at = state()
            lp, sq = torch.zeros(rows, device=DEV), torch.zeros(rows, device=DEV)
            ops.sample_select(xs, ys[:, t], NO_END, PAD, en, cnt, at, t, lp, sq, _sample_ctl(seed, 1, temperature, 1.0), ws, cols=V)
            got[f"sample_select top_k=1 seed={seed} T={temperature}"] = ys[:, t]
            assert not en.any() and int(cnt[0]) == 0 and int(at[0]) == Lmax
        ys, fin, cnt, at = state()                        # K = 1: every row is a video with one beam, score 0, not finished
        sc = torch.zeros(rows, dtype=torch.float32, device=DEV)
        parent = torch.full((rows,), -7, dtype=torch.int32, device=DEV)
        bws = torch.full((ops.beam_select_workspace_bytes(dtype, rows, 1, V) // 4,), float("nan"), dtype=torch.float32, device=DEV)
        ops.beam_select(xs, rows, 1, sc, fin, parent, ys[:, t], NO_END, PAD, cnt, at, t, bws, cols=V)
        got["beam_select K=1"] = ys[:, t]
        torch.cuda.synchronize()
        assert parent.cpu().tolist() == list(range(rows)) and not fin.any() and int(cnt[0]) == 0
        for name, tok in got.items():
            assert np.array_equal(tok.cpu().numpy(), want), (name, V, dtype, ldx, tok.cpu().numpy(), want)
