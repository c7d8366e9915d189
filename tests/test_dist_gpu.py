"""Two data-parallel ranks through the REAL kernel schedule on one GPU (gloo moves the CUDA gradient buckets; the
driver's multi-GPU runs use RCCL with the same GradExchange / bucket hooks): every bucket must be complete --
weight gradients from the side stream, bias / LayerNorm gradients from the main stream -- at the moment its hook
fires, the averaged gradients must drive Adam per bucket, and the ranks must end up with identical parameters equal
to a single-process step on the mean gradient."""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


MC = {"modal": ["clip"], "modal_shape": [48], "text_enc_type": "CLIP", "embed_dim": 64, "dropout": 0.0, "loss_beta": 0.5,
      "matching": {"enable_tem": False, "matching_loss": "CSL"}, "activation": "gelu",
      "video_encoder": {"layer": 2, "nhead": 4, "feedforward": 128,
                        "mme": {"temporal": "encoding", "modal_different": True, "do_norm": False, "aggregation": "avg"}, "aoa": False},
      "caption_decoder": {"layer": 2, "nhead": 4, "feedforward": 128, "sce_loss_alpha": 0.5}, "pretrained_model": None}
VOCAB = 301


def _batch(seed, dev):
    g = torch.Generator().manual_seed(seed)
    feats = torch.randn(6, 7, 48, generator=g).to(dev)
    mask = torch.zeros(6, 7, dtype=torch.bool); mask[1, 5:] = True; mask[4, 3:] = True
    ids = torch.randint(3, VOCAB, (6, 9), generator=g); ids[:, 0] = 101; ids[2, 6:] = 0
    return feats, mask.to(dev), ids.to(dev)


def _np_batch(seed):
    f, mk, i = _batch(seed, "cpu")
    return f.numpy(), mk.numpy(), i.numpy()


def _oracle_mean_step(start_sd, ps, world, steps, lr):
    """The CHECKER: per step, the CPU oracle's gradient of every rank's batch, averaged over the ranks (what DDP's reducer
    produces, reference train.py:217-219), then the oracle's Adam (train.py:24-26,126).  Returns (flat mean gradient of the
    first step laid out like the model's flat buffer, parameters after `steps` steps, |mean gradient| > 1e-5 mask per name)."""
    import numpy as np
    import vct_oracle as O
    cfg = O.cfg_from_model_config(MC, VOCAB)
    p = {k: v.detach().cpu().numpy().copy() for k, v in start_sd.items()}
    state, flat1, big = {}, None, None
    for k in range(steps):
        gs = [O.caption_loss_and_grads(p, cfg, *_np_batch(10 + rr + 2 * k))[1] for rr in range(world)]
        g = {n: sum(x[n].astype(np.float64) for x in gs) / world for n in gs[0]}
        if k == 0:
            flat1 = np.zeros(ps.total, np.float64)
            for n, v in g.items():
                flat1[ps.offsets[n]:ps.offsets[n] + v.size] = v.reshape(-1)
            big = {n: np.abs(v) > 1e-5 for n, v in g.items()}
        else:
            big = {n: big[n] & (np.abs(v) > 1e-5) for n, v in g.items()}
        p = O.adam_step(p, {n: v.astype(np.float32) for n, v in g.items()}, state, lr=lr)
    return flat1, p, big


def _worker(rank, world, port, dtype_name, q, sharded=False, executor="eager", check_oracle=False):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "oracle"), os.path.join(root, "tests")):
        sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    import torch.distributed as dist
    from helpers import build_model
    from vct_amd.trainer import CaptionTrainer, FusedAdam, GradExchange
    dist.init_process_group("gloo", rank=rank, world_size=world)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dtype = getattr(torch, dtype_name)
    torch.manual_seed(50 + rank)                       # different init per rank: the constructor broadcast fixes it
    m = build_model(MC, VOCAB, "cuda", dtype)
    m.train()
    opt = FusedAdam(m, lr=1e-3)
    if sharded:       # reduce-scatter -> Adam on the owned half -> all-gather (gloo carries the CUDA buffers on this one-GPU box)
        from vct_amd.comm import C10dColl
        from vct_amd.trainer import ShardedExchange
        ex = ShardedExchange(m, opt, C10dColl())
        assert ex.shard_of(0) is not None and ex.shard_of(0)[2] * world == ex.buckets[0][1] - ex.buckets[0][0]
    else:
        ex = GradExchange(m)
    tr = CaptionTrainer(m, opt, ex, launch_list=(executor == "list"))
    assert tr.use_list == (executor == "list")
    start = m.flat_params.clone()
    start_sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    nsteps = 3 if executor == "list" else 2          # list: eager + record, then two replays
    losses, g_first = [], None
    for k in range(nsteps):
        losses.append(float(tr.step(*_batch(10 + rank + 2 * k, dev))))
        if k == 0:
            torch.cuda.synchronize()
            g_first = m.flat_grads.detach().double().cpu().numpy()
    torch.cuda.synchronize()
    ok_oracle, why = True, []
    if check_oracle:
        # exchanged HIP step vs the CPU oracle: (a) the averaged gradient this rank holds after step 1 (its own shard of every
        # bucket when sharded, everything otherwise) within 1e-3 per bucket -- Adam is scale-invariant, so a wrong 1/world only
        # shows here; (b) the parameter update after all steps where the gradient is not noise, within 2 % of the learning rate
        import numpy as np
        flat1, p_ref, big = _oracle_mean_step(start_sd, m._ps, world, nsteps, 1e-3)
        for i, (a, b) in enumerate(m.grad_buckets()):
            b = min(b, m.caption_param_end)
            if b <= a:
                continue
            lo, hi = a, b
            if sharded and ex.shard_of(i) is not None:
                lo, hi, _n = ex.shard_of(i)
                hi = min(hi, b)
            if hi <= lo:
                continue
            # relative to the WHOLE bucket's gradient (a 1/W shard can be almost empty: a slice of the token-embedding table)
            err = np.linalg.norm(g_first[lo:hi] - flat1[lo:hi]) / max(np.linalg.norm(flat1[a:b]) * ((hi - lo) / (b - a)) ** 0.5, 1e-30)
            if not err < 1e-3:
                per = [(n, round(float(np.linalg.norm(g_first[m._ps.offsets[n]:m._ps.offsets[n] + m._ps.params[n].numel()] -
                                                      flat1[m._ps.offsets[n]:m._ps.offsets[n] + m._ps.params[n].numel()]) /
                                       max(np.linalg.norm(flat1[m._ps.offsets[n]:m._ps.offsets[n] + m._ps.params[n].numel()]), 1e-30)), 4))
                       for n in m._ps.names if lo <= m._ps.offsets[n] < hi]
                gg, ff = g_first[lo:hi], flat1[lo:hi]
                why.append(("grad", i, lo, hi, float(err), [x for x in per if x[1] > 1e-3][:3],
                            "norms", float(np.linalg.norm(gg)), float(np.linalg.norm(ff)), "cos", float(gg @ ff / (np.linalg.norm(gg) * np.linalg.norm(ff)))))
            ok_oracle &= bool(err < 1e-3)
        sd = m.state_dict()
        for n, ref in p_ref.items():
            if n not in big or n.endswith("pe") or n.endswith("pos_embedding"):
                continue
            upd = sd[n].detach().cpu().numpy().astype(np.float64) - start_sd[n].cpu().numpy()
            upd_ref = ref.astype(np.float64) - start_sd[n].cpu().numpy()
            worst = float(np.abs(upd - upd_ref)[big[n]].max(initial=0.0))
            if not worst < 2e-5:
                why.append(("update", n, worst))
            ok_oracle &= bool(worst < 2e-5)
    gathered = [torch.empty_like(m.flat_params) for _ in range(world)]
    dist.all_gather(gathered, m.flat_params)
    same = all(torch.equal(gathered[0], g) for g in gathered)
    ok_ref = True
    if rank == 0 and world == 2:     # (more ranks: gloo's reduction order is not the host's running sum -> the oracle check stands in)
        # single process: the two ranks' gradients computed one after the other, averaged, one Adam step -- twice
        r = build_model(MC, VOCAB, "cuda", dtype)
        r.train()
        r.flat_params.copy_(start)
        ropt = FusedAdam(r, lr=1e-3)
        for k in range(nsteps):
            acc = torch.zeros_like(r.flat_grads)
            for rr in range(world):
                r._ps.refresh_shadow(force=True)
                r.train_step_kernels(*_batch(10 + rr + 2 * k, dev))
                acc += r.flat_grads
            r.flat_grads.copy_(acc / world)
            ropt.step()
        named = lambda mm: {k: v for k, v in mm.state_dict().items()}
        a, b = named(m), named(r)
        ok_ref = all(torch.equal(a[k], b[k]) for k in a)
    q.put((rank, same, ok_ref and ok_oracle, losses, why[:6]))
    dist.barrier()
    dist.destroy_process_group()


def _run_ranks(world, dtype_name, sharded, executor):
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, dtype_name, q, sharded, executor, dtype_name == "float32"))
             for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=400) for _ in range(world))
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    for rank, same, ok_ref, losses, why in res:
        assert same, "ranks ended with different parameters"
        assert ok_ref, f"rank {rank}: exchanged step differs from the single-process step on the mean gradient / from the CPU oracle: {why}"
        assert all(l == l and l > 0 for l in losses)
    assert res[0][3] != res[1][3]            # the ranks did see different batches


@pytest.mark.parametrize("sharded,executor", [(False, "eager"), (True, "eager"), (True, "list")])
@pytest.mark.parametrize("dtype_name", ["float32", "bfloat16"])
def test_two_ranks_one_gpu_step_equals_mean_gradient_step(dtype_name, sharded, executor):
    """executor 'list': the exchanged step recorded ONCE (collectives included, as host commands of the list for gloo) and
    replayed -- the executor bench.py uses at N > 1.  float32 also checks the exchanged step against the CPU oracle: the mean
    of the two ranks' oracle gradients and the oracle's Adam."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    _run_ranks(2, dtype_name, sharded, executor)


@pytest.mark.parametrize("dtype_name", ["float32", "bfloat16"])
def test_four_ranks_one_gpu_sharded_recorded_step(dtype_name):
    """World 4 through the real kernel schedule: vct_adam_step on real 1/4 slices of every bucket (offsets that are not the
    bucket start), the reduce-scatter payload offsets, the all-gather of the masters and the refresh of the derived copies
    (bf16 shadow, W_g^T) behind it, recorded as a launch list and replayed.  float32: the exchanged step against the ORACLE
    (mean of the four ranks' oracle gradients + oracle Adam); every dtype: all ranks end with identical parameters."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    _run_ranks(4, dtype_name, True, "list")


def test_bench_two_rank_control_flow_on_one_gpu(tmp_path):
    """bench.py --gpus 2 --full as the driver launches it (one process per rank, RANK / WORLD_SIZE / MASTER_* from the env), with
    both ranks on the ONE GPU of the test box and gloo as the process group: barrier, MAX-reduce of the elapsed time, rank-0-only
    JSON line, whole-job value = 2 x per-GPU batch x steps / time, sharded exchange through the torch.distributed collectives,
    the exchange's brackets (--full), and --dump-outputs after the moments were gathered from both ranks."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    port = _free_port()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   VCT_DIST_BACKEND="gloo")
        procs.append(subprocess.Popen([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "2",
                                       "--batch", "16", "--full", "--no-cpu-baseline", "--no-decode", "--dump-outputs", str(tmp_path)],
                                      env=env, cwd=root,
                                      stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    outs = [p.communicate(timeout=600) for p in procs]
    assert all(p.returncode == 0 for p in procs), [o[1][-2000:] for o in outs]
    lines0 = [l for l in outs[0][0].splitlines() if l.startswith("{")]
    lines1 = [l for l in outs[1][0].splitlines() if l.startswith("{")]
    assert len(lines0) == 1 and not lines1                        # ONE JSON line, from rank 0
    d = json.loads(lines0[0])
    assert d["n_gpus"] == 2 and d["steps"] == 3 and d["scaling"] == "weak"
    assert d["config"]["global_batch"] == 32 and d["config"]["grad_exchange"].startswith("sharded/")
    assert d["config"]["executor"] == "list"                      # N > 1 runs the recorded launch list by default
    assert abs(d["value"] - 32 * 3 / (d["ms_per_step"] * 3e-3)) < 0.01 * d["value"]
    assert d["loss"] == d["loss"] and "cpu_baseline" not in d
    # exchange evidence fields (rccl_ranks is null here: gloo carries the buckets on this one-GPU box)
    c = d["comm"]
    assert c["kind"].startswith("sharded/") and "rccl_ranks" in c and c["exposed_wait_ms"] is not None
    assert len(c["bucket_ms_on_comm_stream"]) >= 4 and all(v is not None and v > 0 for v in c["bucket_ms_on_comm_stream"])
    import numpy as np
    loss = np.load(tmp_path / "loss.npy")
    assert loss.dtype == np.float32 and loss.tolist() == [d["loss"]]
    m = np.load(tmp_path / "adam_exp_avg.cap_decoder.generator.weight.npy")
    e = np.load(tmp_path / "adam_exp_avg.video_encoder.transformer_encoder.layers.0.linear1.weight.npy")
    # rank 1 steps its half of every bucket's moments: without the gather rank 0 would write zeros there
    assert m.dtype == np.float32 and np.isfinite(m).all() and (m != 0).mean() > 0.9 and (e != 0).mean() > 0.9
