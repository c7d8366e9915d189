"""MMT4Caption -- drop-in for the reference's model/MMT4Caption.py:15-211: the caption task on every executor, the video-text
matching task ('match') and both together ('cross') on the eager one.

Same constructor (`MMT4Caption(cfg['model'], device)`), `forward(video_feats, video_masks, captions)`,
`caption_forward`, `match_forward`, `cross_forward`, `greedy_decode`, `mode`, attributes (`cap_preprocessor`, `cap_decoder`,
`video_encoder`, `matching`, `device`, `f_type`) and state_dict keys.  All parameters live in ONE
flat fp32 buffer laid out in gradient-ready order (with a matching flat gradient buffer and a bf16
shadow), so the data-parallel gradient exchange and the optimizer work on contiguous slices."""
import os
from typing import List, Optional

import torch
import torch.nn as nn

from .. import ops
from ..engine import ParamSet, first_input, memory_len
from .CapDecoder import CapDecoder, grad_ready_order_decoder
from .CapPreprocessor import CapPreprocessor
from .Matching import Matching, TextEncoder, check_text_feats
from .MMEncoder import HMMEncoder, MultiModalEncoder

_DTYPES = {"bf16": torch.bfloat16, "bfloat16": torch.bfloat16, "fp32": torch.float32, "float32": torch.float32}


class _CaptionFn(torch.autograd.Function):
    """loss = caption_forward(...) as ONE autograd node: forward = encoder + decoder + loss kernels,
    backward = the explicit reverse schedule; gradients land in the flat gradient buffer."""

    @staticmethod
    def forward(ctx, model, feats, mask, ids, *params):
        ctx.model = model
        return model._forward_loss(feats, mask, ids, model.training)[0]

    @staticmethod
    def backward(ctx, gloss):
        m = ctx.model
        m._backward()
        m._ps.install_grads()
        if not m._unit_loss_grad:
            m._ps.gflat.mul_(gloss)
        return (None, None, None, None) + (None,) * len(m._ps.names)


class _MatchFn(torch.autograd.Function):
    """loss = match_forward(...) as ONE autograd node: encoder + matching head forward, the reverse schedule in backward.  The
    decoder is never entered and its parameters get no gradient (.grad stays None, as in the reference)."""

    @staticmethod
    def forward(ctx, model, feats, mask, text, *params):
        ctx.model = model
        ctx.st = model._match_forward_kernels(feats, mask, text, model.training, backward=True)
        return ctx.st["loss"][0].clone()

    @staticmethod
    def backward(ctx, gloss):
        m = ctx.model
        m._match_backward_kernels(ctx.st)
        a = m.encoder_param_begin
        m._ps.install_grads()
        if not m._unit_loss_grad:
            m._ps.gflat[a:].mul_(gloss)
        return (None, None, None, None) + (None,) * len(m._ps.names)


class _CrossFn(torch.autograd.Function):
    """(loss, cap_loss, match_loss) = cross_forward(...) as ONE autograd node; only `loss` is differentiable (train.py:133-136
    backpropagates nothing else)."""

    @staticmethod
    def forward(ctx, model, feats, mask, ids, text, *params):
        ctx.model = model
        loss, cap, match, ctx.st = model._cross_forward_kernels(feats, mask, ids, text, model.training, backward=True)
        out = (loss.clone().reshape(()), cap.clone().reshape(()), match.clone().reshape(()))
        ctx.mark_non_differentiable(out[1], out[2])
        return out

    @staticmethod
    def backward(ctx, gloss, _gcap, _gmatch):
        m = ctx.model
        m._cross_backward_kernels(ctx.st)
        m._ps.install_grads()
        if not m._unit_loss_grad:
            m._ps.gflat.mul_(gloss)
        return (None, None, None, None, None) + (None,) * len(m._ps.names)


class MMT4Caption(nn.Module):
    overlap_enc_bwd = True      # encoder backward beside the decoder's tail (A/B switch)
    overlap_dec_prefix = True   # decoder embedding + bottom self-attention beside the encoder forward (A/B switch)

    def __init__(self, model_config: dict, device=torch.device("cuda"), compute_dtype=None):
        super().__init__()
        self.device = device
        self.model_config = model_config
        self.loss_beta = model_config["loss_beta"]
        self.f_type = None
        cd = compute_dtype or model_config.get("compute_dtype") or os.environ.get("VCT_COMPUTE_DTYPE", "bf16")
        self.compute_dtype = _DTYPES[cd] if isinstance(cd, str) else cd

        self.cap_preprocessor = CapPreprocessor(model_config["tokenizer"], device=device,
                                                vocab_size=model_config.get("vocab_size"))
        self.text_encoder = TextEncoder(model_config["text_enc_type"], device=device, dim=model_config.get("text_enc_dim"))
        dec_cfg, enc_cfg = model_config["caption_decoder"], model_config["video_encoder"]
        self.cap_decoder = CapDecoder(
            num_layers=dec_cfg["layer"], embed_dim=model_config["embed_dim"], nhead=dec_cfg["nhead"],
            dim_feedforward=dec_cfg["feedforward"], dropout=model_config["dropout"],
            vocab_size=self.cap_preprocessor.tokenizer.vocab_size, pad_id=self.cap_preprocessor.pad_id,
            sce_loss_alpha=dec_cfg["sce_loss_alpha"], custom_decoder_type=dec_cfg.get("layer_type", None),
            activation=model_config["activation"], device=device, compute_dtype=self.compute_dtype,
            label_smoothing=dec_cfg.get("label_smoothing", 0.0))      # optional key: absent = 0 = the reference's criterion
        enc_type = enc_cfg.get("type", "mme")
        if enc_type not in ("mme", "hmme"):
            raise NotImplementedError(f"video_encoder.type {enc_type!r} is outside the accelerated caption path ('mme' and 'hmme' are on it)")
        mme = enc_cfg["mme"]
        # 'hmme': video_encoder.layer is the per-stream list of depths, the options come from the `mme` block (MMT4Caption.py of the reference)
        self.video_encoder = (HMMEncoder if enc_type == "hmme" else MultiModalEncoder)(
            d_feats=model_config["modal_shape"], d_model=model_config["embed_dim"], nhead=enc_cfg["nhead"],
            dim_feedforward=enc_cfg["feedforward"], num_encoder_layers=enc_cfg["layer"], dropout=model_config["dropout"],
            activation=model_config["activation"], global_type=mme["aggregation"],
            modal_different=mme.get("modal_different", True), temporal_type=mme.get("temporal", "encoding"),
            do_norm=mme.get("do_norm", False), device=device, compute_dtype=self.compute_dtype)
        if model_config.get("matching", None) is not None:
            self.matching = Matching((model_config["embed_dim"], self.text_encoder.dim),
                                     enable_tem=model_config["matching"]["enable_tem"],
                                     loss=model_config["matching"]["matching_loss"],
                                     loss_tem=model_config["matching"].get("temperature", None), device=device)
        self._enc_type = enc_type
        self._ps: Optional[ParamSet] = None
        self._unit_loss_grad = False
        self._seed = None
        self._pending_enc_bwd = None      # train_step_kernels(defer_join=True): the encoder backward, not enqueued yet
        self._mem = None                  # the encoder memory of the last caption forward
        self._build_flat()
        if model_config.get("text_enc_weights"):
            # optional: a CLIP state dict on disk -> the text tower on our kernels (text.py).  It still needs a tokenizer
            # (tower.tokenize = clip.tokenize) before it can take strings; ids work as they are.
            from ..text import ClipTextTower
            self.install_text_encoder(ClipTextTower.from_file(model_config["text_enc_weights"], device, compute_dtype=self.compute_dtype))

    def install_text_encoder(self, tower):
        """Make `tower` (text.ClipTextTower) the producer of the matching task's sentence features: model.text_encoder(captions)
        then runs it.  Its weights stay outside this module's parameters and state_dict (the reference's TextEncoder is no module)."""
        if int(tower.dim) != int(self.text_encoder.dim):
            raise ValueError(f"the text tower produces {tower.dim}-dimensional features, the model's text encoder (and the matching "
                             f"head) is sized for {self.text_encoder.dim}: set model.text_enc_dim")
        mine, theirs = torch.device(self.device), torch.device(tower.device)
        if theirs.type != mine.type or (None not in (mine.index, theirs.index) and mine.index != theirs.index):
            raise ValueError(f"the text tower is on {tower.device}, the model on {self.device}")
        self.text_encoder.backend = tower
        return tower

    # ---- flat parameter storage --------------------------------------------------------------------
    def _build_flat(self):
        named = dict(self.named_parameters())
        order = (grad_ready_order_decoder("cap_decoder.", self.cap_decoder.cfg["layers"]) +
                 self.video_encoder._order("video_encoder.", self.video_encoder.cfg["layers"], self.video_encoder.num_modal,
                                           self.video_encoder.cfg["temporal_type"], self.video_encoder.do_norm))
        order += [n for n in named if n not in set(order)]   # matching.* (not on the caption path)
        dev = named[order[0]].device
        self._ps = ParamSet([(n, named[n]) for n in order], dev, self.compute_dtype, no_shadow=("cap_decoder.tgt_to_emb.weight",))
        if self._seed is None or self._seed.device != dev:
            self._seed = torch.tensor([torch.initial_seed() & 0x7FFFFFFF], dtype=torch.int32, device=dev)
        self.cap_decoder._bind(self._ps, "cap_decoder.", self._seed, self._build_flat)
        self.video_encoder._bind(self._ps, "video_encoder.", self._seed, self._build_flat)

    def _apply(self, fn, *a, **k):
        out = super()._apply(fn, *a, **k)
        if self._ps is not None and not self._ps.intact():
            self._build_flat()
        return out

    @property
    def flat_params(self) -> torch.Tensor:
        return self._ps.flat

    @property
    def flat_grads(self) -> torch.Tensor:
        return self._ps.gflat

    @property
    def grads_valid(self) -> bool:
        """True when every `.grad` / `flat_grads` element is the gradient of the LAST backward, as after the reference's
        `loss.backward()` (train.py:125).  False after a CaptionTrainer step that stepped the weight matrices inside their
        weight-gradient GEMMs without storing the gradients (single GPU, bf16, FusedAdam -- the default there): bias, LayerNorm and
        embedding gradients are current, the 2-D weights' are stale.  `CaptionTrainer(..., keep_weight_grads=True)` keeps all valid."""
        return self._ps.weight_grads_valid

    def check_grads_valid(self):
        """Raise if the weight-matrix gradients are stale (call before gradient clipping / logging / hooks that read .grad)."""
        if not self._ps.weight_grads_valid:
            raise RuntimeError("the last CaptionTrainer.step() stepped the weight matrices inside their weight-gradient GEMMs and did not "
                               "store those gradients: .grad / flat_grads of 2-D weights are stale; construct the trainer with "
                               "keep_weight_grads=True (or set VCT_FUSE_ADAM_KEEP_GRAD=1) to keep them")

    def grad_buckets(self):
        """Contiguous [start, end) element ranges of the flat gradient buffer in the order the backward
        pass completes them: generator | decoder norm + top layer | ... | decoder layer 0 | token embedding |
        encoder norm + top layer | ... | encoder layer 0 + unify (+ parameters outside the caption path).  The hierarchical encoder
        has no stack-final norm: its first bucket starts at the top layer's norm2."""
        ps, o = self._ps, self._ps.offsets
        enc = self.video_encoder
        Ld, Le = self.cap_decoder.cfg["layers"], enc.cfg["layers"]
        enc_layers = "video_encoder." + enc.layers_at
        enc_first = "video_encoder." + enc.final_norm + "weight" if enc.final_norm else f"{enc_layers}{Le - 1}.norm2.weight"
        cuts = [0, o["cap_decoder.decoder.norm.weight"]]
        cuts += [o[f"cap_decoder.decoder.layers.{l}.norm3.weight"] for l in reversed(range(Ld - 1))]
        cuts += [o["cap_decoder.tgt_to_emb.weight"], o[enc_first]]
        cuts += [o[f"{enc_layers}{l}.norm2.weight"] for l in reversed(range(Le - 1))]
        cuts.append(ps.total)
        return [(cuts[i], cuts[i + 1]) for i in range(len(cuts) - 1)]

    def bucket_index(self, kind: str, layer: int = 0) -> int:
        """Index into grad_buckets(): kind in {'generator', 'dec_layer', 'embedding', 'enc_layer'}; `layer` is the
        layer whose backward just finished."""
        Ld, Le = self.cap_decoder.cfg["layers"], self.video_encoder.cfg["layers"]
        if kind == "generator":
            return 0
        if kind == "dec_layer":
            return 1 + (Ld - 1 - layer)
        if kind == "embedding":
            return 1 + Ld
        if kind == "enc_layer":
            return 2 + Ld + (Le - 1 - layer)
        raise ValueError(kind)

    # ---- engine-level forward/backward (no autograd) ------------------------------------------------
    def _forward_loss(self, feats, mask, ids, training, want_logits=False):
        """feats / mask: one tensor (one modality) or one tensor per modality (mask: a list or None)."""
        if not self._ps.intact():
            self._build_flat()
        self._ps.refresh_shadow()
        enc, dec = self.video_encoder._engine(), self.cap_decoder._engine()
        B, Te = first_input(feats).shape[0], memory_len(feats)      # Te: the encoder's memory rows per sample
        ops.tap("layers_fwd", 0)      # bench.py north_star bracket: input cast .. decoder final LayerNorm (main stream)
        if self.overlap_dec_prefix and dec.dev.type == "cuda" and dec.overlap_dw:
            # token embedding + the decoder's bottom self-attention block do not need the encoder: side stream, beside it
            dec.forward_prefix(B, Te, ids, training)
        mem = self._mem = enc.forward(feats, mask, training)      # (kept for the matching head of the cross task)
        loss, logits = dec.forward(mem, B, Te, ids, training, want_logits=want_logits)
        self.cap_decoder._publish_attn(dec)
        return loss, logits

    @property
    def encoder_param_begin(self) -> int:
        """Flat offset where the encoder's parameters (and whatever follows them) start: everything before it -- generator,
        decoder stack, token embedding -- has its final gradient before the encoder backward has finished."""
        return self.grad_buckets()[2 + self.cap_decoder.cfg["layers"]][0]

    @property
    def caption_param_end(self) -> int:
        """Flat offset where the parameters OUTSIDE the caption path (matching.*) start -- the end of what the caption
        task's optimizer owns (reference train.py:24: filter(requires_grad) after mode('caption'))."""
        ps = self._ps
        for n in ps.names:
            if not (n.startswith("cap_decoder.") or n.startswith("video_encoder.")):
                return ps.offsets[n]
        return ps.total

    def join_backward(self):
        """train_step_kernels(defer_join=True) leaves the encoder backward un-enqueued: enqueue it (side stream) if that
        has not happened yet, then make the main stream wait for it."""
        self.launch_encoder_backward()
        self.cap_decoder._engine().join_side()

    def launch_encoder_backward(self, main: bool = False):
        """main: enqueue it on the CURRENT stream (the caller has joined the side stream: d(memory) is final) -- for the one-launch
        sample-stationary backward, which takes whole compute units and gains nothing from running beside other kernels."""
        fn, self._pending_enc_bwd = self._pending_enc_bwd, None
        if fn is not None:
            fn(main)

    def encoder_backward_is_one_launch(self) -> bool:
        enc = self.video_encoder._engine()
        return enc.ss_bwd_ok()

    def _backward(self, bucket_ready=None, join: bool = True, fold=None):
        """fold = (B, N, Te): the decoder ran on B*N rows over the memory of B videos fanned out N times (_forward_scst) -- its
        d(memory) [B*N*Te, d] is summed over each video's N blocks (ops.group_sum) on the stream that carries it, before the
        encoder backward reads it."""
        hook = None
        if bucket_ready is not None:
            def hook(kind, layer=0):
                bucket_ready(self.bucket_index(kind, layer))
        dec, enc = self.cap_decoder._engine(), self.video_encoder._engine()

        def folded(dmem):      # on the current stream, where d(memory) is final
            if fold is None:
                return dmem
            B, N, Te = fold
            return ops.group_sum(dmem, enc.cur.get("scst.dmem", (B * Te, dmem.shape[1]), dmem.dtype), B, N, Te)
        if self.overlap_enc_bwd and dec.dev.type == "cuda" and dec.overlap_dw:
            # the encoder's backward only needs d(memory): it runs on the side stream beside the decoder's bottom
            # self-attention backward and the embedding gradient (two chains of small kernels share the chip)
            def launch(dmem, dmem_point, main=False):
                if main:
                    enc.backward(folded(dmem), hook, join=False)
                    return
                side = dec.ensure_side()
                ops.sync_wait(dmem_point, side)                   # d(memory) final (its last accumulate is on `side` itself)
                enc.main_stream = torch.cuda.current_stream()     # (EncoderEngine.enc_dw_main: upper layers' weight-gradient groups go there)
                try:
                    with torch.cuda.stream(side):
                        enc.backward(folded(dmem), hook)
                finally:
                    enc.main_stream = None

            def on_dmem(dmem, dmem_point):
                if join:
                    launch(dmem, dmem_point)
                else:      # the caller enqueues its own main-stream work first (the host launches ~35 kernels here)
                    self._pending_enc_bwd = lambda main=False: launch(dmem, dmem_point, main)
            dec.backward(hook, on_dmem_ready=on_dmem, join=join)  # join: ends with the main stream joining the side stream
        else:
            dmem = dec.backward(hook)
            enc.backward(folded(dmem), hook)

    def train_step_kernels(self, feats, mask, ids: torch.Tensor, bucket_ready=None, defer_join: bool = False) -> torch.Tensor:
        """Fast path used by the trainer and bench: forward + backward as one static kernel schedule
        (hipGraph-capturable, no autograd tape).  Gradients are WRITTEN (not accumulated) into the flat
        gradient buffer, whose views are installed as `.grad`.  Returns the loss tensor [1].
        feats / mask: a tensor (one modality) or a list with one tensor per modality (mask: a list or None)."""
        loss, _ = self._forward_loss(feats, mask, ids, self.training)
        self._backward(bucket_ready, join=not defer_join)     # defer_join: the caller calls join_backward() itself
        opt = self._ps.dw_adam                                # the optimizer epilogue consumed the weight gradients unless told to store them
        self._ps.weight_grads_valid = opt is None or bool(opt.keep_grads)
        return loss

    # ---- self-critical sequence training: N sampled captions per video, one weight (advantage) per caption --------------------
    def _forward_scst(self, feats, mask, ids, N: int, training, seq_w=None, score=False, want_logits=False):
        """_forward_loss with the encoder on the B videos and the decoder on the B*N id rows (row b*N + n = sample n of video b, the
        sampler's layout): the memory rows are copied B -> B*N into an engine buffer (N = 1: used as they are)."""
        if not self._ps.intact():
            self._build_flat()
        self._ps.refresh_shadow()
        enc, dec = self.video_encoder._engine(), self.cap_decoder._engine()
        B, Te = first_input(feats).shape[0], memory_len(feats)
        ops.tap("layers_fwd", 0)
        if self.overlap_dec_prefix and dec.dev.type == "cuda" and dec.overlap_dw:
            dec.forward_prefix(B * N, Te, ids, training)
        mem = self._mem = enc.forward(feats, mask, training)
        if N > 1:
            d = mem.shape[1]
            rep = dec.buf((B * N, Te, ids.shape[1])).get("scst.mem", (B * N * Te, d), mem.dtype)
            rep.view(B, N, Te, d).copy_(mem.reshape(B, 1, Te, d).expand(-1, N, -1, -1))
            mem = rep
        loss, logits = dec.forward(mem, B * N, Te, ids, training, want_logits=want_logits, seq_w=seq_w, score=score)
        self.cap_decoder._publish_attn(dec)
        return loss, logits

    def _check_scst_ids(self, feats, ids, num_samples):
        B, N = first_input(feats).shape[0], int(num_samples)
        if N < 1:
            raise ValueError(f"num_samples must be >= 1, got {num_samples}")
        if ids.dim() != 2 or ids.dtype != torch.int64 or ids.shape[0] != B * N or ids.shape[1] < 2:
            raise ValueError(f"ids must be int64 [B * num_samples = {B * N}, L >= 2] (row b*N + n = sample n of video b), got "
                             f"{ids.dtype} {tuple(ids.shape)}")
        return B, N

    def train_step_kernels_scst(self, feats, mask, ids: torch.Tensor, seq_w: torch.Tensor, num_samples: int = 1) -> torch.Tensor:
        """The self-critical step as one static kernel schedule, no autograd tape.  feats / mask: B videos (as train_step_kernels);
        ids int64 [B*N, L], row b*N + n = sample n of video b (sample_decode_ids' layout, pads after each row's end token); seq_w
        fp32 [B*N] on the device, the advantage of each row.  The encoder runs once on B, its memory is fanned out to the B*N
        decoder rows, the loss is -(sum over non-pad tokens of seq_w[row] * log p(token)) / (number of non-pad tokens)
        (DecoderEngine.forward: sce_loss_alpha and the RCE term do not enter), and the decoder's d(memory) is summed over each
        video's N samples before the encoder backward.  The cross-attention takes no memory mask, so nothing else is fanned out;
        N = 1 launches neither the copy nor the sum.  Gradients are WRITTEN (not accumulated) into the flat gradient buffer, like
        train_step_kernels.  Returns the loss tensor [1]."""
        B, N = self._check_scst_ids(feats, ids, num_samples)
        if seq_w.dtype != torch.float32 or seq_w.numel() != B * N or seq_w.device != ids.device or not seq_w.is_contiguous():
            raise ValueError(f"seq_w must be contiguous fp32 [{B * N}] on {ids.device}, got {seq_w.dtype} {tuple(seq_w.shape)} on {seq_w.device}")
        loss, _ = self._forward_scst(feats, mask, ids, N, self.training, seq_w=seq_w.reshape(-1))
        self._backward(None, join=True, fold=(B, N, memory_len(feats)) if N > 1 else None)
        opt = self._ps.dw_adam
        self._ps.weight_grads_valid = opt is None or bool(opt.keep_grads)
        return loss

    @torch.no_grad()
    def score_captions(self, video_feats, video_masks, ids: torch.Tensor, num_samples: int = 1):
        """Teacher-forced log-probabilities of given captions, forward only (no logits gradient, dropout off, gradient buffers
        untouched).  ids int64 [B*num_samples, L] (row b*N + n belongs to video b).  Returns (seq_logp fp32 [B*num_samples], the sum
        over each row's non-pad targets, and tok_logp fp32 [B*num_samples, L-1], log p(ids[:, t+1] | ids[:, :t+1]), 0 where the
        target is pad)."""
        feats, mask = self._video_inputs(video_feats, video_masks)
        B, N = self._check_scst_ids(feats, ids, num_samples)
        self._forward_scst(feats, mask, ids, N, False, score=True)
        tok = self.cap_decoder._engine().cur.t["tok_logp"].view(B * N, ids.shape[1] - 1).clone()
        return tok.sum(1), tok

    # ---- reference API -----------------------------------------------------------------------------
    def _video_inputs(self, video_feats, video_masks):
        """The reference's per-modality lists -> what the engines take: the tensor itself for one modality (a bare tensor is
        accepted too), the list for several."""
        n = self.video_encoder.num_modal
        if isinstance(video_feats, torch.Tensor):
            if n > 1:
                raise ValueError(f"the model has {n} feature streams: pass one tensor per stream, not a single tensor")
            return video_feats, (video_masks[0] if isinstance(video_masks, (list, tuple)) else video_masks)
        if n == 1:
            return video_feats[0], (video_masks[0] if video_masks is not None else None)
        if len(video_feats) != n or (video_masks is not None and len(video_masks) != n):
            raise ValueError(f"expected {n} feature streams (and as many masks, or None), got {len(video_feats)}")
        return list(video_feats), (list(video_masks) if video_masks is not None else None)

    def forward(self, video_feats: List[torch.Tensor], video_masks: List[torch.Tensor], captions, text_feats=None):
        """text_feats (match / cross): fp32 [B, text_encoder.dim] on the model's device; None = self.text_encoder(captions)."""
        if self.f_type == "caption":
            return self.caption_forward(video_feats, video_masks, captions)
        if self.f_type == "match":
            return self.match_forward(video_feats, video_masks, captions, text_feats)
        if self.f_type == "cross":
            return self.cross_forward(video_feats, video_masks, captions, text_feats)
        raise ValueError

    # ---- the matching task ('match') and both tasks ('cross'): eager executor, 'mme' encoder ------------------------------------
    def check_task(self, task: Optional[str] = None):
        """Refuse, before any device work, what the matching task is not built for."""
        task = self.f_type if task is None else task
        if task not in ("match", "cross"):
            return
        if getattr(self, "matching", None) is None:
            raise ValueError(f"task {task!r} needs the matching head: model_config['matching'] is None")
        if self._enc_type == "hmme":
            raise NotImplementedError(f"task {task!r} with video_encoder.type 'hmme' is not built: the hierarchical encoder's agg_feats is "
                                      "one scalar per sample ([B]), which the matching head's v_proj cannot take")

    def _text_feats(self, captions, text_feats, B):
        if text_feats is None:
            text_feats = self.text_encoder(captions)
        return check_text_feats(text_feats, B, self.text_encoder.dim, self.flat_params.device)

    def _match_forward_kernels(self, feats, mask, text, training, backward, mem=None):
        """Encoder forward (unless `mem` is given: the cross task's caption forward made it), the aggregation rows, the head."""
        if mem is None:
            if not self._ps.intact():
                self._build_flat()
            self._ps.refresh_shadow()
            mem = self.video_encoder._engine().forward(feats, mask, training)
        B, Te = first_input(feats).shape[0], memory_len(feats)
        agg = self.matching._buf("agg", (B, mem.shape[1]), mem.device)
        ops.match_agg_fwd(mem, agg, B, Te)
        st = self.matching.head_forward(text, agg, backward=backward)
        st["B"], st["Te"], st["mem"] = B, Te, mem
        return st

    def _head_backward_kernels(self, st):
        """d(match loss) into the matching.* slice of the flat gradient buffer; returns d(match loss)/d(agg) fp32 [B, d]."""
        mt, g = self.matching, self._ps.g
        dagg = mt._buf("dagg", tuple(st["agg"].shape), st["agg"].device)
        if mt.v_proj is not None:
            dagg = mt.head_backward(st, dagg, g["matching.v_proj.weight"], g["matching.v_proj.bias"])
        else:
            dagg = mt.head_backward(st, dagg)
        if mt.loss_fn.learned:
            ops.axpby(g["matching.loss_fn.temperature"], st["dtemp"], 1.0)
        return dagg

    def _match_backward_kernels(self, st, hook=None):
        enc = self.video_encoder._engine()
        dagg = self._head_backward_kernels(st)
        dmem = enc.cur.get("match.dmem", tuple(st["mem"].shape), st["mem"].dtype)
        ops.match_agg_bwd(dmem, dagg, st["B"], st["Te"], 0.0, empty=True)     # every row written: no zero fill, the buffer is not read
        enc.backward(dmem, hook)

    def _cross_forward_kernels(self, feats, mask, ids, text, training, backward):
        cap_loss, _ = self._forward_loss(feats, mask, ids, training)
        st = self._match_forward_kernels(feats, mask, text, training, backward, mem=self._mem)
        beta = float(self.loss_beta)
        loss = ops.axpby(self.matching._buf("cross_loss", (1,), cap_loss.device), cap_loss.reshape(1), beta, st["loss"], 1.0 - beta)
        return loss, cap_loss, st["loss"], st

    def _cross_backward_kernels(self, st, hook=None):
        dec, enc = self.cap_decoder._engine(), self.video_encoder._engine()
        beta = float(self.loss_beta)
        dmem = dec.backward(hook)                                  # the non-overlapped branch: ends with the side stream joined
        ops.scale(self._ps.gflat[:self.encoder_param_begin], beta)   # the caption task's decoder-side gradients, times beta
        dagg = self._head_backward_kernels(st)
        a = self.caption_param_end
        if a < self._ps.total:
            ops.scale(self._ps.gflat[a:], 1.0 - beta)              # matching.*: only the match loss reaches them
        ops.match_agg_bwd(dmem, dagg, st["B"], st["Te"], beta)     # beta * d(cap)/d(memory) + (1 - beta) * d(match)/d(memory), in place
        enc.backward(dmem, hook)

    def train_step_kernels_match(self, feats, mask, text_feats: torch.Tensor) -> torch.Tensor:
        """The match task's step as one static kernel schedule, no autograd tape: encoder forward, aggregation rows, head, head
        backward, d(memory) (only the aggregation rows are non-zero), encoder backward.  Gradients of the encoder and of matching.*
        are WRITTEN into the flat gradient buffer; the decoder engine is never entered and its slice is not written.  Returns the
        loss tensor [1]."""
        self.check_task("match")
        text = check_text_feats(text_feats, first_input(feats).shape[0], self.text_encoder.dim, self.flat_params.device)
        st = self._match_forward_kernels(feats, mask, text, self.training, backward=True)
        self._match_backward_kernels(st)
        self._ps.weight_grads_valid = True
        return st["loss"]

    def train_step_kernels_cross(self, feats, mask, ids: torch.Tensor, text_feats: torch.Tensor):
        """Both tasks in one step: the caption forward, the head on the same memory, the decoder backward, its gradients times
        loss_beta, the head backward, beta * d(cap)/d(memory) + (1 - beta) * d(match)/d(memory), the encoder backward.  Same contract
        as train_step_kernels.  Returns (loss, cap_loss, match_loss), three device tensors [1]."""
        self.check_task("cross")
        text = check_text_feats(text_feats, first_input(feats).shape[0], self.text_encoder.dim, self.flat_params.device)
        loss, cap, match, st = self._cross_forward_kernels(feats, mask, ids, text, self.training, backward=True)
        self._cross_backward_kernels(st)
        self._ps.weight_grads_valid = True
        return loss, cap, match

    def match_forward(self, video_feats, video_masks, captions, text_feats=None):
        """MMT4Caption.py:126-133 of the reference: the contrastive loss between the text features and the encoder's agg_feat."""
        self.check_task("match")
        feats, mask = self._video_inputs(video_feats, video_masks)
        text = self._text_feats(captions, text_feats, first_input(feats).shape[0])
        if not torch.is_grad_enabled():
            return self._match_forward_kernels(feats, mask, text, self.training, backward=False)["loss"][0].clone()
        return _MatchFn.apply(self, feats, mask, text, *[self._ps.params[n] for n in self._ps.names]).reshape(())

    @torch.no_grad()
    def embed_videos(self, video_feats, video_masks) -> torch.Tensor:
        """The video side of the matching head for retrieval: encoder forward in eval mode, the aggregation rows, v_proj when the
        head has one -> a new fp32 [B, text_encoder.dim] tensor.  NOT normalised (the retrieval kernels normalise); no autograd.
        Refuses what the match task refuses (check_task)."""
        self.check_task("match")
        feats, mask = self._video_inputs(video_feats, video_masks)
        if not self._ps.intact():
            self._build_flat()
        self._ps.refresh_shadow()
        mem = self.video_encoder._engine().forward(feats, mask, False)
        B, Te = first_input(feats).shape[0], memory_len(feats)
        mt = self.matching
        agg = ops.match_agg_fwd(mem, torch.empty(B, mem.shape[1], dtype=torch.float32, device=mem.device), B, Te)
        if mt.v_proj is None:
            return agg
        out = torch.empty(B, mt.vt_shape[1], dtype=torch.float32, device=mem.device)
        ops.gemm(agg, mt.v_proj.weight.data, out, bias=mt.v_proj.bias.data)
        return out

    def cross_forward(self, video_feats, video_masks, captions, text_feats=None):
        """MMT4Caption.py:135-147 of the reference: (loss_beta * cap_loss + (1 - loss_beta) * match_loss, cap_loss, match_loss);
        the two task losses come back detached."""
        self.check_task("cross")
        text_ts, _text_mask_ts = self.cap_preprocessor(captions)
        feats, mask = self._video_inputs(video_feats, video_masks)
        text = self._text_feats(captions, text_feats, first_input(feats).shape[0])
        if not torch.is_grad_enabled():
            loss, cap, match, _ = self._cross_forward_kernels(feats, mask, text_ts, text, self.training, backward=False)
            return loss[0].clone(), cap[0].clone(), match[0].clone()
        return _CrossFn.apply(self, feats, mask, text_ts, text, *[self._ps.params[n] for n in self._ps.names])

    def caption_forward(self, video_feats, video_masks, captions):
        text_ts, _text_mask_ts = self.cap_preprocessor(captions)
        feats, mask = self._video_inputs(video_feats, video_masks)
        if not torch.is_grad_enabled():
            return self._forward_loss(feats, mask, text_ts, self.training)[0][0].clone()
        return _CaptionFn.apply(self, feats, mask, text_ts, *[self._ps.params[n] for n in self._ps.names]).clone().reshape(())

    @torch.no_grad()
    def greedy_decode(self, video_feat: List[torch.Tensor], video_masks: Optional[List[torch.Tensor]] = None,
                      max_len: int = 30, return_attn: bool = False, controls=None):
        """return_attn: (captions, maps fp32 [B, layers, steps, Te]) -- see greedy_decode_ids.  controls: a
        decode.GenerationControls (minimum length, no-repeat n-gram ban, repetition penalty, banned ids)."""
        if return_attn:
            ys, maps = self.greedy_decode_ids(video_feat, video_masks, max_len, return_attn=True, controls=controls)
            return self._ids_to_captions(ys), maps
        return self._ids_to_captions(self.greedy_decode_ids(video_feat, video_masks, max_len, controls=controls))

    def _ids_to_captions(self, ys: torch.Tensor) -> List[str]:
        end_id = self.cap_preprocessor.end_id
        result = []
        for idx_cap in ys.tolist():
            end_count = -1
            for i, idx in enumerate(idx_cap):
                if idx == end_id:
                    end_count = i
                    break
            idx_cap = idx_cap[1:end_count]   # reference quirk kept: without [SEP] the last token is dropped
            toks = self.cap_preprocessor.tokenizer.convert_ids_to_tokens(idx_cap)
            result.append(self.cap_preprocessor.tokenizer.convert_tokens_to_string(toks))
        return result

    @torch.no_grad()
    def greedy_decode_ids(self, video_feat, video_masks=None, max_len: int = 30, kv_cache: bool = True,
                          use_graphs: bool = True, return_attn: bool = False, controls=None):
        """The id matrix ys [B, <=max_len] of MMT4Caption.greedy_decode (MMT4Caption.py:159-172).
        kv_cache=False runs the reference's O(L^2) algorithm (full decoder re-run per token).
        return_attn (KV cache only; any model, with or without caption_decoder.layer_type): (ys, maps) with maps fp32
        [B, layers, ys.shape[1] - 1, Te], row t-1 = the head-averaged cross-attention of the token consumed at step t
        (predict_video.py --vis_attn).  controls: a decode.GenerationControls; every step's arg-max is then taken from the processed
        logits (semantics: decode.GenerationControls), on either path."""
        if return_attn and not kv_cache:
            raise ValueError("return_attn needs the KV-cached decode (kv_cache=True)")
        was_training = self.training
        self.eval()
        try:
            from .. import decode
            feats, mask = self._video_inputs(video_feat, video_masks)
            if kv_cache:
                return decode.greedy_decode_ids(self, feats, mask, max_len, use_graphs=use_graphs, return_attn=return_attn,
                                                controls=controls)
            return decode.greedy_decode_ids_reference_algorithm(self, feats, mask, max_len, controls=controls)
        finally:
            self.train(was_training)

    @torch.no_grad()
    def beam_decode(self, video_feat: List[torch.Tensor], video_masks: Optional[List[torch.Tensor]] = None, beam_size: int = 5,
                    max_len: int = 30, length_penalty: float = 1.0, return_attn: bool = False, controls=None) -> List[str]:
        """Beam-search captions, one string per video (the reference's beam_decode is `pass`, MMT4Caption.py:186); ids -> text
        as greedy_decode.  Semantics: decode.beam_decode_ids.  return_attn=True raises ValueError: attention maps would have to
        follow the beams' parent back-track (greedy decoding returns them).  controls: a decode.GenerationControls; the beam scores
        are then log-probabilities under the controlled distribution."""
        from ..decode import _no_beam_attn
        _no_beam_attn(return_attn)
        return self._ids_to_captions(self.beam_decode_ids(video_feat, video_masks, beam_size, max_len, length_penalty, controls=controls))

    @torch.no_grad()
    def beam_decode_ids(self, video_feat, video_masks=None, beam_size: int = 5, max_len: int = 30, length_penalty: float = 1.0,
                        kv_cache: bool = True, use_graphs: bool = True, return_all: bool = False, return_attn: bool = False,
                        controls=None):
        """The best beam's id matrix [B, <=max_len] (return_all: (ids [B, K, L'], final scores [B, K])) of beam_decode.
        kv_cache=False runs the reference algorithm (full decoder re-run per token, host-side selection).  controls: a
        decode.GenerationControls, on either path."""
        from ..decode import _no_beam_attn
        _no_beam_attn(return_attn)
        was_training = self.training
        self.eval()
        try:
            from .. import decode
            feats, mask = self._video_inputs(video_feat, video_masks)
            if kv_cache:
                return decode.beam_decode_ids(self, feats, mask, beam_size, max_len, length_penalty,
                                              use_graphs=use_graphs, return_all=return_all, controls=controls)
            return decode.beam_decode_ids_reference_algorithm(self, feats, mask, beam_size, max_len, length_penalty,
                                                              return_all=return_all, controls=controls)[0]
        finally:
            self.train(was_training)

    @torch.no_grad()
    def sample_decode(self, video_feat: List[torch.Tensor], video_masks: Optional[List[torch.Tensor]] = None, num_samples: int = 1,
                      max_len: int = 30, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0, seed=None,
                      kv_cache: bool = True, controls=None) -> List[List[str]]:
        """Sampled captions: for every video a list of num_samples strings (ids -> text as greedy_decode).  Semantics:
        decode.sample_decode_ids.  controls: a decode.GenerationControls; tokens are then drawn from the controlled distribution."""
        ids = self.sample_decode_ids(video_feat, video_masks, num_samples, max_len, temperature, top_k, top_p, seed, kv_cache,
                                     controls=controls)
        B, N = ids.shape[0], ids.shape[1]
        flat = self._ids_to_captions(ids.reshape(B * N, -1))
        return [flat[b * N:(b + 1) * N] for b in range(B)]

    @torch.no_grad()
    def sample_decode_ids(self, video_feat, video_masks=None, num_samples: int = 1, max_len: int = 30, temperature: float = 1.0,
                          top_k: int = 0, top_p: float = 1.0, seed=None, kv_cache: bool = True, use_graphs: bool = True,
                          return_logp: bool = False, controls=None):
        """The id table [B, num_samples, <=max_len] of sample_decode (return_logp: (ids, seq_logp fp32 [B, num_samples])).
        kv_cache=False runs the reference algorithm (full decoder re-run per token, host-side selection with the same draws).
        controls: a decode.GenerationControls; return_logp is then the log-probability under the controlled distribution."""
        from .. import decode
        decode._check_sample_args(num_samples, temperature, top_k, top_p)
        was_training = self.training
        self.eval()
        try:
            feats, mask = self._video_inputs(video_feat, video_masks)
            kw = dict(max_len=max_len, num_samples=num_samples, temperature=temperature, top_k=top_k, top_p=top_p, seed=seed,
                      return_logp=return_logp, controls=controls)
            if kv_cache:
                return decode.sample_decode_ids(self, feats, mask, use_graphs=use_graphs, **kw)
            return decode.sample_decode_ids_reference_algorithm(self, feats, mask, **kw)[0]
        finally:
            self.train(was_training)

    def mode(self, forward_type="caption") -> None:
        self.f_type = forward_type
        matching = getattr(self, "matching", None)
        mparams = list(matching.parameters()) if matching is not None else []
        if forward_type == "caption":
            flags = (True, False)
        elif forward_type == "match":
            flags = (False, True)
        elif forward_type == "cross":
            flags = (True, True)
        else:
            raise ValueError
        for p in self.cap_decoder.parameters():
            p.requires_grad = flags[0]
        for p in mparams:
            p.requires_grad = flags[1]
