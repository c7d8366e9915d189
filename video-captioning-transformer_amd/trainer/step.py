"""The step executor (CaptionTrainer: eager, recorded launch list or captured hipGraph; the match / cross tasks: eager only) and the
epoch loop."""
from typing import Optional
import os

import torch
import torch.distributed as dist

from .. import ops
from ..engine import first_input, stage_inputs, static_inputs
from ..utils import capture_graph
from .clip import GradClipper, clip_settings_of
from .exchange import GradExchange, ShardedExchange
from .optim import FusedAdam, owned_range


class CaptionTrainer:
    """One object = the reference's `model(...) -> zero_grad -> backward -> step` loop body
    (train.py:123-126) on the kernel fast path, with the gradient exchange folded into backward.

    Executors of the ~100-launch step (single GPU, FusedAdam):
      * eager (default off the GPU fast path): Python issues every launch through ctypes;
      * launch_list=True: the step is recorded ONCE per input shape into a C-side launch list (ops.LaunchList:
        every launch with its stream, every cross-stream edge) and re-issued by one C call per step -- eager
        two-stream semantics without the Python/ctypes cost per launch;
      * use_graph=True: the step is captured into a hipGraph (bitwise equal, but replay serialises the two streams).
    Inputs are copied into static buffers; the dropout seed, the Adam step counter and the Adam hyper-parameters live
    in device memory, so every replay sees fresh values.  Recordings are dropped when an activation buffer of THIS model had
    to grow (engine/params.py: StepContext.generation), because they bake device pointers."""

    def __init__(self, model, optimizer, exchange: Optional[GradExchange] = None, use_graph: bool = False,
                 launch_list: Optional[bool] = None, keep_weight_grads: Optional[bool] = None, loss_stats: Optional[bool] = None):
        """loss_stats: True / False sets model.cap_decoder.loss_stats (None leaves it): the caption loss then also leaves the
        un-smoothed NLL and the token accuracy on the device at label_smoothing 0 (last_nll, last_token_acc); with label_smoothing > 0
        they are always there.
        keep_weight_grads: on the single-GPU bf16 FusedAdam path the 2-D weights are stepped inside their weight-gradient GEMMs and
        their gradients are NOT stored (model.grads_valid is False after a step; the reference leaves valid .grad after backward,
        train.py:125).  True stores them as well (for clipping, logging, hooks; costs the 4 B per parameter the fusion saved);
        None: the VCT_FUSE_ADAM_KEEP_GRAD environment switch (default off).
        Clipping needs none of this: set max_grad_norm / clip_grad_value on the optimizer (FusedAdam(..., max_grad_norm=...),
        train.optimizer.max_grad_norm, or param_groups[0]) and the step clips on the device (trainer/clip.py); the fusion is then off
        and every gradient is stored.  After such a step: last_grad_norm, last_clip_coef, grad_norms()."""
        self.model, self.opt, self.ex = model, optimizer, exchange
        fused = self._fused = isinstance(optimizer, FusedAdam)
        # the task the optimizer was built for (FusedAdam remembers model.f_type; a torch optimizer's filter(requires_grad) followed it)
        self.task = (optimizer.task if fused else model.f_type) or "caption"
        self._asked = (bool(use_graph), bool(launch_list))
        self._check_task(self.task)
        if keep_weight_grads is not None and fused:
            optimizer.set_keep_grads(bool(keep_weight_grads))
        model._unit_loss_grad = True
        single = (exchange is None or not exchange.active) and fused
        # a launch list can also carry the exchange when every collective is recordable: stream work of the library's own RCCL
        # communicator, or host commands of the list (comm.C10dColl under ops.host_call: the one-GPU multi-rank tests)
        listable = single or (isinstance(exchange, ShardedExchange) and getattr(exchange.coll, "recordable", False))
        self.use_graph = bool(use_graph) and single
        self.use_list = (bool(launch_list) if launch_list is not None else False) and listable and not self.use_graph
        # recordings per input shape, as (recording, its loss tensor): launch lists / captured graphs, both replayed by .replay()
        self._lists = {}
        self._graphs = {}
        self._static = {}                 # per input shape: the static input buffers the recordings read
        # per input shape, Vis decoders only: the attention-map views that shape's recording writes.  Every shape shares the engine's
        # grow-only buffers, so the views Python published for the LAST shape it ran have another shape's dimensions
        self._attn = {}
        self._gen = None                  # the buffer generation (engine.StepContext) the recordings were made at
        # the caption loss's by-products (label smoothing / loss_stats): fp32 [2] in the decoder engine's buffer set, per input shape
        if loss_stats is not None:
            model.cap_decoder.loss_stats = bool(loss_stats)
        self._stats = None                # the (NLL, token accuracy) buffer the LAST step wrote, or None
        self._stats_of = {}               # per input shape: the buffer that shape's recording writes
        self._stats_mode = self._loss_stats_mode()
        if single and model.flat_grads.is_cuda:
            # this trainer (zero_grad implicit, no exchange, no in-place averaging) is the only writer of the gradient buffer
            model.cap_decoder._engine().exclusive_grads = True
        # single GPU: per-bucket Adam on the side stream was measured SLOWER (3.28 vs 3.14 ms/step: the 6.5 TB/s
        # optimizer pass steals HBM bandwidth from the GEMMs it overlaps), so it is opt-in; with a gradient exchange
        # Adam always runs per bucket as each all-reduce lands (it overlaps the wire, not the GEMMs)
        self.overlap_adam = False
        # single GPU, FusedAdam, bf16: every weight matrix is stepped in the epilogue of its own weight-gradient GEMM (FusedAdam.
        # enable_dw_fusion); the hook is installed only WHILE this trainer enqueues a step (a plain loss.backward() outside it must
        # keep producing gradients and nothing else)
        # (match / cross: off -- cross scales the gradients before they are consumed, match gains nothing worth the risk)
        self._fuse_base = self.fuse_adam = bool(single and optimizer.fuse_dw_default and self.task == "caption"
                                                and model._ps.compute_dtype == torch.bfloat16 and model.flat_grads.is_cuda)
        # gradient clipping (optimizer.param_groups[0]: max_grad_norm / clip_grad_value; trainer/clip.py).  Off unless one is set: no
        # launch is added or moved.  On: the norm needs every gradient in memory before any parameter is stepped, so the optimizer
        # leaves the weight-gradient GEMMs (fuse_adam off) and the caption step takes the plain branch -- backward with both streams
        # joined, the clipper's two or three launches, the optimizer.
        self.clipper = None
        self._clip_mode = None
        self._sync_clip()

    # ---- NLL and token accuracy beside a smoothed loss --------------------------------------------------------------------------------
    def _loss_stats_mode(self):
        dec = self.model.cap_decoder
        return (float(dec.cfg.get("label_smoothing", 0.0)), bool(dec.loss_stats))

    def _sync_loss_stats(self):
        """Recordings bake which loss entry point a step launches (and its smoothing, a launch scalar): drop them when
        cap_decoder.loss_stats or the smoothing was changed since.  Host-only."""
        mode = self._loss_stats_mode()
        if mode != self._stats_mode:
            self._stats_mode = mode
            self.drop_recordings()

    def _published_stats(self):
        return self.model.cap_decoder._engine().last_loss_stats

    @property
    def last_nll(self):
        """0-dim device fp32: the un-smoothed negative log-likelihood per non-pad token of the last caption step (fairseq's
        nll_loss), a view of the engine's buffer that the next step rewrites; no synchronisation.  None unless that step ran the
        smoothed entry point: label_smoothing > 0, or loss_stats."""
        return None if self._stats is None else self._stats[0]

    @property
    def last_token_acc(self):
        """0-dim device fp32: the share of non-pad tokens whose label held the row's largest logit (a tie counts) in the last caption
        step.  None under last_nll's conditions."""
        return None if self._stats is None else self._stats[1]

    # ---- gradient clipping -------------------------------------------------------------------------------------------------------------
    def _sync_clip(self):
        """Follow the clipping settings of optimizer.param_groups[0] (a scheduler, load_state_dict or the user may have written
        them): validate, switch the step's shape when clipping was turned on or off (recordings are dropped: they bake the launches),
        upload the thresholds when they changed.  Host-only otherwise; called before every step, outside any capture."""
        mode, max_norm, max_value = clip_settings_of(self.opt)
        if mode != self._clip_mode:
            if mode is not None and self.ex is not None and self.ex.active:
                raise NotImplementedError("gradient clipping with an active gradient exchange is not built: the sharded path steps "
                                          "each bucket before the global norm exists")
            if mode is not None and self.clipper is None:
                begin, end = (self.opt.begin, self.opt.end) if self._fused else owned_range(self.model, self.task)
                self.clipper = GradClipper(self.model, begin, end)
            self._clip_mode = mode
            self.fuse_adam = self._fuse_base and mode is None
            self.drop_recordings()
        if mode is not None:
            self.clipper.sync(max_norm, max_value)

    def _clip(self):
        """The clipper's launches on the current stream, between the backward (every stream joined) and the optimizer."""
        if self._clip_mode is not None:
            self.clipper.enqueue()

    @property
    def last_grad_norm(self):
        """0-dim device fp32: the global L2 norm of the last step's gradients BEFORE clipping (what clip_grad_norm_ returns); a view
        of the clipper's state, rewritten by the next step.  None unless max_grad_norm is set."""
        return self.clipper.state[0] if self._clip_mode == "norm" else None

    @property
    def last_clip_coef(self):
        """0-dim device fp32: the factor the last step's gradients were multiplied by (1 = not clipped).  None unless max_grad_norm is set."""
        return self.clipper.state[1] if self._clip_mode == "norm" else None

    def grad_norms(self):
        """(parameter names, device fp32 [n]): the L2 norm of every parameter's gradient before clipping -- a by-product of the
        last step's norm pass.  None unless max_grad_norm is set."""
        return (list(self.clipper.names), self.clipper.seg_norm) if self._clip_mode == "norm" else None

    def _check_task(self, task):
        """The matching task runs on the eager executor of one process: refuse the rest loudly, before any device work."""
        if task not in ("match", "cross"):
            return
        self.model.check_task(task)
        if self._asked[0] or self._asked[1]:
            raise NotImplementedError(f"task {task!r} runs on the eager executor only: use_graph / launch_list recordings of it are not built")
        if self.ex is not None and self.ex.active:
            raise NotImplementedError(f"task {task!r} is single-process only: the gradient exchange of it is not built")

    def _step_task(self, feats, mask, ids, text_feats):
        """match / cross: train_step_kernels_* then the optimizer over the task's range (gradients stay valid: model.grads_valid)."""
        m = self.model
        if text_feats is None:
            if m.text_encoder.backend is None or ids is None:
                raise ValueError(f"task {self.task!r}: pass text_feats (fp32 [B, {m.text_encoder.dim}] on the model's device)")
            text_feats = m.text_encoder(ids)        # an installed encoder (MMT4Caption.install_text_encoder) takes the captions
        ops.tap("step", 0)
        if not self._fused:
            m._ps.masters_written()
        else:
            m._ps.refresh_shadow()
        if self.task == "match":
            out = m.train_step_kernels_match(feats, mask, text_feats)
        else:
            out = m.train_step_kernels_cross(feats, mask, ids, text_feats)      # (the loss_beta mix of the gradients is part of it)
        self._clip()
        self.opt.step()
        if m.training and m.video_encoder.cfg["dropout"] > 0:
            ops.advance_seed(m._seed)
        ops.tap("step", 1)
        self._stats = self._published_stats() if self.task == "cross" else None
        return out

    def _check_scst(self, num_samples, baseline):
        """Self-critical training runs on the eager executor of one process, on the caption task: refuse the rest loudly, before
        any device work."""
        if self._asked[0] or self._asked[1]:
            raise NotImplementedError("scst_step runs on the eager executor only: build the trainer without use_graph / launch_list")
        if self.ex is not None and self.ex.active:
            raise NotImplementedError("scst_step is single-process only: the gradient exchange of it is not built")
        if (self.model.f_type or "caption") != "caption" or self.task != "caption":
            raise ValueError(f"scst_step trains the caption task: model.mode({self.model.f_type!r}), optimizer built for {self.task!r}")
        if int(num_samples) < 1:
            raise ValueError(f"num_samples must be >= 1, got {num_samples}")
        if baseline not in ("mean_others", "greedy"):
            raise ValueError(f"baseline must be 'mean_others' or 'greedy', got {baseline!r}")
        if baseline == "mean_others" and int(num_samples) < 2:
            raise ValueError("baseline 'mean_others' is the leave-one-out mean of the other samples: it needs num_samples >= 2")

    def scst_step(self, feats, mask, reward_fn, vids=None, *, num_samples: int = 5, baseline: str = "mean_others", max_len: int = 30,
                  temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0, seed=None):
        """One self-critical sequence training step (policy gradient on a sentence-level reward): sample num_samples captions per
        video (model.sample_decode_ids, no grad), score them on the host (reward_fn(ids int64 [B, N, L] CPU, vids) -> float [B, N]:
        the step's one host sync), turn the rewards into advantages (rewards.advantages: 'mean_others' = leave-one-out, 'greedy' =
        the reward of one greedy_decode caption per video), then model.train_step_kernels_scst on the samples with one advantage
        per caption, and the optimizer.  The optimizer-in-the-weight-gradient-GEMM fusion stays off for this step.  vids: what
        reward_fn gets as video ids (default 0 .. B-1).  seed: the sampler's (None: one draw from torch's generator).
        Returns dict(loss = device tensor [1], reward_mean, baseline_mean = floats, ids = int64 [B, N, L] on the device).

        A reward object with `on_device = True` (rewards.CiderD.to_device()) keeps the whole step on the device: reward_fn(ids,
        vids) is enqueued behind the sampler on the current stream (the greedy baseline is scored by the same kernel on
        [B, 1, L]), ops.scst_advantages writes seq_w, and the step never copies ids to the host nor waits for the reward.  On
        THAT path reward_mean and baseline_mean are 0-dim DEVICE tensors (fp32): floats would put the host sync back; convert
        them when you need the numbers (scst_epoch does it once per epoch).  max_len above 65 is a ValueError there, before any
        launch (the reward kernel takes the start column + 64 tokens)."""
        self._check_scst(num_samples, baseline)
        self._sync_clip()
        self._stats = None                      # the policy-gradient loss (ops.wce_loss) ignores label smoothing and leaves no NLL / accuracy
        if getattr(reward_fn, "on_device", False):
            return self._scst_step_device(feats, mask, reward_fn, vids, int(num_samples), baseline, max_len, temperature, top_k, top_p,
                                          seed)
        from ..rewards import advantages
        import numpy as np
        m, N = self.model, int(num_samples)
        if self._fused:
            self.opt.sync_hyper()
            m._ps.refresh_shadow()
        else:
            m._ps.masters_written()               # a torch optimizer wrote the fp32 masters: re-cast the shadow before decoding
        B = first_input(feats).shape[0]
        vids = list(range(B)) if vids is None else list(vids)
        ids = m.sample_decode_ids(feats, mask, num_samples=N, max_len=max_len, temperature=temperature, top_k=top_k, top_p=top_p,
                                  seed=seed)
        greedy = m.greedy_decode_ids(feats, mask, max_len=max_len) if baseline == "greedy" else None
        r = np.asarray(reward_fn(ids.cpu(), vids), np.float32)          # the host sync
        if r.shape != (B, N):
            raise ValueError(f"reward_fn must return [B = {B}, N = {N}] rewards, got {r.shape}")
        if greedy is not None:
            base = np.asarray(reward_fn(greedy.cpu().view(B, 1, -1), vids), np.float32).reshape(B)
            adv = advantages(r, base)
        else:
            adv = advantages(r, "mean_others")
            base = r - adv
        seq_w = torch.from_numpy(np.ascontiguousarray(adv.reshape(-1))).to(ids.device)
        loss = m.train_step_kernels_scst(feats, mask, ids.view(B * N, -1), seq_w, N)
        self._clip()
        self.opt.step()
        if m.training and m.video_encoder.cfg["dropout"] > 0:
            ops.advance_seed(m._seed)
        # (a copy: the engine's loss buffer is rewritten by the next forward, score_captions included)
        return dict(loss=loss.clone(), reward_mean=float(r.mean()), baseline_mean=float(base.mean()), ids=ids)

    def _scst_step_device(self, feats, mask, reward_fn, vids, N, baseline, max_len, temperature, top_k, top_p, seed):
        """scst_step with a device-resident reward: same stages, nothing on the host between the sampler and the train step."""
        from ..rewards import DEVICE_MAX_LEN
        if int(max_len) > 1 + DEVICE_MAX_LEN:
            raise ValueError(f"scst_step: a device reward scores the start column + at most {DEVICE_MAX_LEN} tokens, got max_len = {max_len}")
        m = self.model
        B = first_input(feats).shape[0]
        vids = list(range(B)) if vids is None else list(vids)
        if len(vids) != B:
            raise ValueError(f"scst_step: {B} videos and {len(vids)} video ids")
        rows = getattr(reward_fn, "video_rows", None)
        if rows is not None:
            rows(vids)                            # KeyError for an unknown video, and the id upload, ahead of the sampler's queue
        if self._fused:
            self.opt.sync_hyper()
            m._ps.refresh_shadow()
        else:
            m._ps.masters_written()
        ids = m.sample_decode_ids(feats, mask, num_samples=N, max_len=max_len, temperature=temperature, top_k=top_k, top_p=top_p,
                                  seed=seed)
        greedy = m.greedy_decode_ids(feats, mask, max_len=max_len) if baseline == "greedy" else None
        r = reward_fn(ids, vids)
        if not torch.is_tensor(r) or tuple(r.shape) != (B, N) or r.dtype != torch.float32 or r.device != ids.device:
            raise ValueError(f"a device reward_fn must return fp32 [B = {B}, N = {N}] on {ids.device}, got {getattr(r, 'shape', type(r))}")
        base = reward_fn(greedy.view(B, 1, -1), vids).view(B) if greedy is not None else None
        seq_w, _, means = ops.scst_advantages(r.contiguous(), base)
        loss = m.train_step_kernels_scst(feats, mask, ids.view(B * N, -1), seq_w, N)
        self._clip()
        self.opt.step()
        if m.training and m.video_encoder.cfg["dropout"] > 0:
            ops.advance_seed(m._seed)
        return dict(loss=loss.clone(), reward_mean=means[0], baseline_mean=means[1], ids=ids)

    # A/B switch (single GPU): the whole Adam pass after the joined backward instead of 86 % of it beside the encoder backward
    adam_after_backward = os.environ.get("VCT_ADAM_TAIL", "0") == "1"
    warm_streams = os.environ.get("VCT_WARM_STREAMS", "1") != "0"

    def _step_kernels(self, feats, mask, ids):
        if not self.fuse_adam:
            return self._step_kernels_body(feats, mask, ids)
        self.opt.enable_dw_fusion(True)
        self.opt.begin_step()
        try:
            return self._step_kernels_body(feats, mask, ids)
        finally:
            self.opt.enable_dw_fusion(False)

    def _step_kernels_body(self, feats, mask, ids):
        m = self.model
        fused = self._fused
        ops.tap("step", 0)
        if not fused:
            m._ps.masters_written()               # a torch optimizer wrote the fp32 masters: re-cast the shadow
        else:
            m._ps.refresh_shadow()                # FusedAdam keeps the shadow current (first step: cast once)
        exchanging = self.ex is not None and self.ex.active
        if exchanging and isinstance(self.ex, ShardedExchange):
            # reduce-scatter -> Adam on the owned shard -> all-gather, per bucket, on the communicator's stream
            loss = m.train_step_kernels(feats, mask, ids, bucket_ready=self.ex.bucket_ready)
            self.ex.finish()
        elif exchanging:
            loss = m.train_step_kernels(feats, mask, ids, bucket_ready=self.ex.bucket_ready)
            if fused:                             # Adam per bucket as its averaged gradient lands
                self.ex.finish(on_bucket_done=self.opt.step_range)
                self.opt.finish_ranges()
            else:
                self.ex.finish()
                self.opt.step()
        elif self._clip_mode is not None:
            # clipping: the whole backward with both streams joined, the norm over every gradient, then the optimizer
            loss = m.train_step_kernels(feats, mask, ids)
            self._clip()
            self.opt.step()
        elif fused and self.overlap_adam and first_input(feats).is_cuda:
            # single GPU: Adam on each gradient bucket the moment backward completes it, on the side stream, so the
            # 1.4 GB optimizer pass hides under the rest of backward instead of trailing it
            buckets = m.grad_buckets()
            ctx = m._ps.ctx

            def hook(i):
                side = ctx.side
                if side is None:
                    self.opt.step_range(*buckets[i])
                    return
                ops.stream_wait(side, None)
                with torch.cuda.stream(side):
                    self.opt.step_range(*buckets[i])
            loss = m.train_step_kernels(feats, mask, ids, bucket_ready=hook)   # zero_grad is implicit: grads are overwritten
            if ctx.side is not None:
                ops.stream_wait(None, ctx.side)
            self.opt.finish_ranges()
        elif fused and first_input(feats).is_cuda and m.overlap_enc_bwd and not self.adam_after_backward:
            # the encoder backward is still running on the side stream when the decoder's tail is done: Adam on everything
            # but the encoder (86 % of the parameters at cfg-B) fills that gap on the main stream, the rest follows the join
            loss = m.train_step_kernels(feats, mask, ids, defer_join=True)
            a = m.encoder_param_begin
            # the decoder layers' weight gradients and the d(memory) GEMMs were issued on the SIDE stream: Adam reads
            # those gradients and rewrites the weights those kernels read, so the main stream joins the side stream first
            # (it is idle here: the encoder backward has not been enqueued yet)
            m.cap_decoder._engine().join_side()
            if m.encoder_backward_is_one_launch():
                # the sample-stationary backward takes whole compute units: alone on the main stream, ahead of the optimizer's pass; its
                # weight-gradient GEMMs (side stream) then run beside that pass
                m.launch_encoder_backward(main=True)
            ops.tap("adam", 0)
            self.opt.step_range(0, a)            # enqueued BEFORE the encoder backward: one launch vs ~35
            ops.tap("adam", 1)
            m.launch_encoder_backward()
            m.join_backward()
            self.opt.step_range(a, m._ps.total)
            self.opt.finish_ranges()
        else:
            loss = m.train_step_kernels(feats, mask, ids)
            self.opt.step()
        if self.warm_streams and first_input(feats).is_cuda:
            # the next step begins with the two sample-stationary stack launches, which stream these packed weights chunk by chunk with
            # two chunks of prefetch: behind the optimizer's passes (1.4 GB of traffic through the memory-side cache) every chunk is an
            # HBM miss
            for stream in m._ps.packed.values():
                ops.warm(stream.t)
        if m.training and m.video_encoder.cfg["dropout"] > 0:
            ops.advance_seed(m._seed)
        ops.tap("step", 1)
        return loss

    def _fresh_shadow(self):
        """Replays skip _step_kernels, which is where the bf16 shadow / transposed copies follow the fp32 masters: if the
        masters were written outside FusedAdam since the last step (load_state_dict, load_weights, restoring the best
        checkpoint), re-cast them eagerly on the current stream before the replay (host-only version-stamp check otherwise)."""
        self.model._ps.refresh_shadow()

    def drop_recordings(self):
        """Forget every recorded launch list / captured graph (they are re-made on the next step of each shape): needed after
        anything that changes WHAT a step launches, e.g. ops.taps_enable(...)."""
        self._lists.clear()
        self._graphs.clear()
        self._attn.clear()
        self._stats_of.clear()

    def _static_inputs(self, key, feats, mask, ids):
        s = self._static.get(key)
        if s is None:
            s = self._static[key] = (static_inputs(feats), static_inputs(mask), ids.clone())
        else:
            # a caller that already works in the static buffers (adopt_inputs) skips the staging copies: three small device copies
            # and the launch gaps around them are ~35 us at the head of a 2.4 ms step
            stage_inputs(s[0], feats, non_blocking=True)
            if mask is not None:
                stage_inputs(s[1], mask, non_blocking=True)
            if s[2].data_ptr() != ids.data_ptr():
                s[2].copy_(ids, non_blocking=True)
        return s

    def _input_key(self, feats, mask, ids):
        if isinstance(feats, (list, tuple)):       # one tensor per modality
            return (tuple((tuple(f.shape), f.dtype) for f in feats), None if mask is None else tuple(tuple(m.shape) for m in mask),
                    tuple(ids.shape), self.model.training)
        return (tuple(feats.shape), feats.dtype, None if mask is None else tuple(mask.shape), tuple(ids.shape), self.model.training)

    def adopt_inputs(self, feats, mask, ids: torch.Tensor):
        """The trainer's own static input buffers for this shape, initialised with the given batch.  Recorded launch lists and
        captured graphs read their inputs from these buffers, so step() normally copies every batch into them; a producer that
        writes its batches INTO them (a device-side loader, a benchmark with resident data) and passes them to step() has no copy
        left.  Returns (feats, mask, ids) views of the buffers; without a recording executor the inputs are returned unchanged.
        feats / mask: a tensor, or one tensor per modality (mask: that list or None)."""
        if not (self.use_graph or self.use_list):
            return feats, mask, ids
        return self._static_inputs(self._input_key(feats, mask, ids), feats, mask, ids)

    def _check_generation(self):
        """Recordings bake device pointers: drop them when a buffer of this model grew (or a packed stream appeared) since they were made."""
        gen = self.model._ps.ctx.generation
        if self._gen != gen:
            self.drop_recordings()
            self._gen = gen

    def _record_list(self, static):
        ll = ops.LaunchList()
        with ll.record():                           # recording executes nothing
            loss = self._step_kernels(*static)
        return ll, loss

    def _capture_graph(self, static):
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        try:
            with capture_graph(graph):
                loss = self._step_kernels(*static)
        except Exception:                           # capture is an optimisation, never a requirement
            self.use_graph = False
            return None
        return graph, loss

    def step(self, feats, mask, ids: torch.Tensor, text_feats: Optional[torch.Tensor] = None):
        """Returns this rank's loss as a device tensor [1] (no host sync); the cross task: (loss, cap_loss, match_loss).  feats / mask:
        a tensor (one modality), or one tensor per modality (mask: that list or None).  text_feats (match / cross): fp32
        [B, text_encoder.dim]; ids may be None for the match task."""
        task = self.model.f_type or "caption"
        if task != self.task:
            raise ValueError(f"model.mode({task!r}) but the optimizer was built for {self.task!r}: build the optimizer after model.mode(task)")
        if self._fused:
            self.opt.sync_hyper()
        self._sync_clip()
        self._sync_loss_stats()
        if self.fuse_adam:
            # the embedding's live-row table exists and is true before the step is enqueued, recorded or replayed (host-only check
            # unless an optimizer state was loaded or a dense pass ran over the table since the last step)
            self.opt.live_refresh()
        if task != "caption":
            self._check_task(task)
            return self._step_task(feats, mask, ids, text_feats)
        if not (self.use_graph or self.use_list):
            loss = self._step_kernels(feats, mask, ids)
            self._stats = self._published_stats()
            return loss
        self._check_generation()
        key = self._input_key(feats, mask, ids)
        static = self._static_inputs(key, feats, mask, ids)
        cache, record = (self._lists, self._record_list) if self.use_list else (self._graphs, self._capture_graph)
        hit = cache.get(key)
        if hit is None:
            # first step of this shape: run it eagerly on the static copies (allocates every buffer), then record the same
            # schedule; later calls replay the recording
            eager_loss = self._step_kernels(*static).clone()
            self._stats = self._published_stats()
            self._check_generation()                # the eager step allocated: older recordings are stale, this one is not made yet
            hit = record(static)
            if hit is not None:
                cache[key] = hit
                if self.model.cap_decoder.custom_decoder_type is not None:
                    self._attn[key] = self.model.cap_decoder.attn_weights
                self._stats_of[key] = self._stats
            return eager_loss
        recording, loss = hit
        self._fresh_shadow()
        recording.replay()
        if key in self._attn:                       # a replay runs no Python forward: publish THIS shape's views of the maps it wrote
            self.model.cap_decoder.attn_weights = self._attn[key]
        self._stats = self._stats_of.get(key)
        self.model._ps.shadow_replayed()            # the replayed optimizer rewrote the shadow
        return loss


def _to_device(model, v_feats, v_masks):
    dev = model.flat_params.device
    if model.video_encoder.num_modal > 1:      # every modality (MMEncoder.forward takes the lists)
        feats = [f.to(dev, non_blocking=True) for f in v_feats]
        mask = [m.to(dev, non_blocking=True) for m in v_masks] if v_masks is not None else None
    else:
        feats = v_feats[0].to(dev, non_blocking=True)
        mask = v_masks[0].to(dev, non_blocking=True) if v_masks is not None else None
    return feats, mask


def train_epoch(model, optimizer, dataloader, mode: str = "caption", exchange: Optional[GradExchange] = None,
                log_every: int = 0, text_feats_fn=None):
    """reference train.py:113-148.  `dataloader` yields (v_feats, v_masks, captions, vids) with the reference's layouts (lists of
    tensors; captions = id rows or strings).  Returns the epoch-mean of the all-rank mean loss ('caption', 'match': a float;
    'cross': (loss, cap_loss, match_loss)) -- one device->host sync per epoch instead of one per step.
    text_feats_fn(captions, vids) -> fp32 [B, text_encoder.dim] (match / cross); without it model.text_encoder(captions)."""
    if mode not in ("caption", "match", "cross"):
        raise ValueError(f"unknown task {mode!r}")
    model.train()
    model.mode(mode)
    trainer = CaptionTrainer(model, optimizer, exchange)
    dev = model.flat_params.device
    total = torch.zeros(3 if mode == "cross" else 1, device=dev)
    n = 0
    for v_feats, v_masks, captions, vids in dataloader:
        feats, mask = _to_device(model, v_feats, v_masks)
        if mode == "caption":
            ids, _ = model.cap_preprocessor(captions)
            total += trainer.step(feats, mask, ids)
        else:
            text = text_feats_fn(captions, vids) if text_feats_fn is not None else model.text_encoder(captions)
            text = text.to(dev, non_blocking=True) if torch.is_tensor(text) else text
            ids = model.cap_preprocessor(captions)[0] if mode == "cross" else None
            out = trainer.step(feats, mask, ids, text)
            total += torch.cat(out) if mode == "cross" else out
        n += 1
    if exchange is not None and exchange.world > 1:
        dist.all_reduce(total, op=dist.ReduceOp.SUM, group=exchange.group)
        total /= exchange.world
    if mode == "cross":
        return tuple(v / max(n, 1) for v in total.tolist())
    return float(total) / max(n, 1)


def scst_epoch(model, optimizer, dataloader, reward_fn, **kw):
    """One epoch of self-critical sequence training (CaptionTrainer.scst_step on every batch): `dataloader` as train_epoch's,
    reward_fn(ids int64 [B, N, L] CPU, vids) -> float [B, N] (e.g. rewards.CiderD over the training references); **kw: scst_step's
    keywords (num_samples, baseline, max_len, temperature, top_k, top_p, seed).  Returns (mean loss, mean reward) of the epoch.
    With a device reward (reward_fn.on_device, e.g. rewards.CiderD.to_device()) the steps' mean rewards are device scalars: they
    are accumulated on the device (fp64) and read once, at the end of the epoch."""
    model.train()
    model.mode("caption")
    trainer = CaptionTrainer(model, optimizer)
    total = torch.zeros(1, device=model.flat_params.device)
    on_device = bool(getattr(reward_fn, "on_device", False))
    reward, n = (torch.zeros((), dtype=torch.float64, device=model.flat_params.device) if on_device else 0.0), 0
    for v_feats, v_masks, _captions, vids in dataloader:
        feats, mask = _to_device(model, v_feats, v_masks)
        out = trainer.scst_step(feats, mask, reward_fn, vids, **kw)
        total += out["loss"]
        reward += out["reward_mean"]
        n += 1
    return float(total) / max(n, 1), float(reward) / max(n, 1)
