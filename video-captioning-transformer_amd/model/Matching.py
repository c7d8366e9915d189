"""The video-text matching head (reference: model/Matching.py:14-30, model/loss.py:7-67): `v_proj` when the encoder width differs
from the text encoder's, then one of the two CLIP-style symmetric losses.  The head is fp32 end to end: v_proj runs through the
exact-fp32 GEMM in both compute modes, the loss (forward and backward in one call) through csrc/vct_match.hip.

Temperature forms (Matching.loss_fn.temperature):
  * `matching.temperature` in the config: a fixed fp32 scalar -- not a parameter, not in the state_dict; enable_tem is irrelevant;
  * enable_tem without it: a learned nn.Parameter([1.0]), state-dict key `matching.loss_fn.temperature`;
  * neither: the reference never sets the attribute and raises AttributeError in forward.  CSL here runs the reference's own
    (unreachable) else branch -- the plain similarity, no scaling; CSL_WDS cannot be defined without a tau and raises ValueError
    at construction."""
from typing import Callable, List, Optional

import torch
import torch.nn as nn

from .. import ops
from ._params import LinearParams

MAX_BATCH, MAX_TEXT_DIM = 256, 1024


class MatchingLoss(nn.Module):
    """Holds the temperature of ClipSymmetricalLoss ('CSL') / ClipSymmetricalLoss_WithDualSoftmax ('CSL_WDS')."""

    def __init__(self, kind, enable_tem=False, tem=None, device=None):
        super().__init__()
        if kind not in ("CSL", "CSL_WDS"):
            raise ValueError(f"matching_loss {kind!r}: 'CSL' or 'CSL_WDS'")
        self.kind, self.enable_tem = kind, bool(enable_tem)
        if tem is not None:
            self.register_buffer("temperature", torch.tensor([float(tem)], dtype=torch.float32, device=device), persistent=False)
        elif enable_tem is True:
            self.temperature = nn.Parameter(torch.tensor([1.0], dtype=torch.float32, device=device), requires_grad=True)
        else:
            if kind == "CSL_WDS":
                raise ValueError("matching_loss 'CSL_WDS' divides the similarity by a temperature: give matching.temperature or set "
                                 "matching.enable_tem (the reference raises AttributeError in forward for this block)")
            self.temperature = None
        # how the kernel uses the scalar: CSL multiplies by exp(temperature), CSL_WDS divides by it
        self.temp_kind = "div" if kind == "CSL_WDS" else ("exp" if self.temperature is not None else "none")

    @property
    def learned(self) -> bool:
        return isinstance(self.temperature, nn.Parameter)


def check_text_feats(text_feats, B: int, dim: int, device) -> torch.Tensor:
    """The text side of the head: fp32 [B, dim] on the model's device (detached: no gradient flows to it)."""
    if not torch.is_tensor(text_feats) or text_feats.dtype != torch.float32 or text_feats.dim() != 2 \
            or tuple(text_feats.shape) != (B, dim) or text_feats.device.type != torch.device(device).type:
        got = (tuple(text_feats.shape), text_feats.dtype, str(text_feats.device)) if torch.is_tensor(text_feats) else type(text_feats)
        raise ValueError(f"text_feats must be fp32 [{B}, {dim}] on {device}, got {got}")
    if B > MAX_BATCH:
        raise ValueError(f"the matching loss kernels take batches of up to {MAX_BATCH} pairs, got {B}")
    t = text_feats.detach()
    return t if t.is_contiguous() else t.contiguous()


class _HeadFn(torch.autograd.Function):
    """loss = Matching(text, vid) as ONE autograd node (vid_feat, v_proj.weight, v_proj.bias and the learned temperature)."""

    @staticmethod
    def forward(ctx, head, text, vid, *params):
        ctx.head = head
        ctx.st = head.head_forward(text, vid.detach(), backward=True)
        ctx.n = len(params)
        return ctx.st["loss"][0].clone()

    @staticmethod
    def backward(ctx, gloss):
        head, st = ctx.head, ctx.st
        B, d = st["agg"].shape
        dev = st["agg"].device
        out = []
        dagg = dw = db = None
        if head.v_proj is not None:
            dagg = torch.empty(B, d, dtype=torch.float32, device=dev)
            dw, db = torch.empty_like(head.v_proj.weight.data), torch.empty_like(head.v_proj.bias.data)
        dagg = head.head_backward(st, dagg, dw, db)
        g = gloss.to(torch.float32)
        if head.v_proj is not None:
            out += [dw * g, db * g]
        if head.loss_fn.learned:
            out.append(st["dtemp"].clone() * g)
        return (None, None, dagg * g) + tuple(out)


class Matching(nn.Module):
    def __init__(self, vt_shape, enable_tem=False, loss="CSL", loss_tem=None, device=None):
        super().__init__()
        self.vt_shape, self.loss = vt_shape, loss
        if vt_shape[1] % 4 or not 4 <= vt_shape[1] <= MAX_TEXT_DIM:
            raise ValueError(f"text-encoder dimension {vt_shape[1]}: the matching loss kernels take multiples of 4 up to {MAX_TEXT_DIM}")
        self.v_proj = LinearParams(vt_shape[0], vt_shape[1], device) if vt_shape[0] != vt_shape[1] else None
        self.loss_fn = MatchingLoss(loss, enable_tem, loss_tem, device)        # (after v_proj: the flat buffer keeps this order)
        self._bufs = {}

    # ---- the head on device tensors (no autograd) ---------------------------------------------------------------------------------
    def _buf(self, name, shape, device):
        key = (name, tuple(shape), str(device))
        t = self._bufs.get(key)
        if t is None:
            t = self._bufs[key] = torch.empty(shape, dtype=torch.float32, device=device)
        return t

    def head_forward(self, text, agg, backward: bool, want_sim: bool = False):
        """text fp32 [B, Dt] (checked by the caller), agg fp32 [B, d] contiguous.  Enqueues v_proj and the loss kernels; with
        `backward` the loss call also leaves d(loss)/d(vid) and d(loss)/d(temperature) in the state it returns (head_backward reads
        them).  Returns dict(loss [1], sim [B, B] or None, ...); buffers are reused per shape: consume them before the next call."""
        B, d = agg.shape
        Dt, dev = self.vt_shape[1], agg.device
        if d != self.vt_shape[0] or tuple(text.shape) != (B, Dt):
            raise ValueError(f"matching head: video features [{B}, {self.vt_shape[0]}] and text features [{B}, {Dt}] expected, got "
                             f"{tuple(agg.shape)} and {tuple(text.shape)}")
        ws_bytes = ops.match_loss_workspace_bytes(B, Dt)
        if self.v_proj is not None:
            vid = self._buf("vid", (B, Dt), dev)
            ops.gemm(agg, self.v_proj.weight.data, vid, bias=self.v_proj.bias.data)
        else:
            vid = agg
        lf = self.loss_fn
        temp = lf.temperature.data if lf.temperature is not None else None
        st = {"agg": agg, "text": text, "vid": vid, "loss": self._buf("loss", (1,), dev),
              "sim": self._buf("sim", (B, B), dev) if want_sim else None, "dvid": None, "dtemp": None}
        if backward:
            st["dvid"] = self._buf("dvid", (B, Dt), dev)
            st["dtemp"] = self._buf("dtemp", (1,), dev) if temp is not None else None
        ops.match_loss(text, vid, st["loss"], self._buf("ws", (ws_bytes // 4,), dev), kind=lf.kind, temp=temp, temp_kind=lf.temp_kind,
                       dvid=st["dvid"], dtemp=st["dtemp"], sim=st["sim"])
        return st

    def head_backward(self, st, dagg, dw=None, db=None):
        """Returns d(loss)/d(agg) fp32 [B, d]: written into `dagg` through v_proj, or -- without v_proj -- the loss call's own
        d(vid) buffer (dagg is not touched).  d(loss)/d(v_proj) is WRITTEN into dw / db (fp32, the parameters' shapes).  The learned
        temperature's gradient is st['dtemp'] (the loss call wrote it)."""
        if self.v_proj is None:
            return st["dvid"]
        ops.gemm(st["dvid"], self.v_proj.weight.data, dagg, ta=False, tb=False)
        ops.gemm(st["dvid"], st["agg"], dw, ta=True, tb=False, bias_grad=db)
        return dagg

    # ---- reference API ---------------------------------------------------------------------------------------------------------------
    def _params(self):
        ps = [self.v_proj.weight, self.v_proj.bias] if self.v_proj is not None else []
        return ps + ([self.loss_fn.temperature] if self.loss_fn.learned else [])

    def _inputs(self, text_feat, vid_feat):
        if not torch.is_tensor(vid_feat) or vid_feat.dim() != 2 or vid_feat.dtype != torch.float32:
            raise ValueError("vid_feat must be an fp32 [B, embed_dim] tensor")
        text = check_text_feats(text_feat, vid_feat.shape[0], self.vt_shape[1], vid_feat.device)
        return text, vid_feat

    def forward(self, text_feat, vid_feat):
        """Matching.py:27-30: loss_fn(text_feat, v_proj(vid_feat)).  Differentiable w.r.t. vid_feat, v_proj.* and the learned
        temperature; text_feat is detached."""
        text, vid = self._inputs(text_feat, vid_feat)
        vid_c = vid if vid.is_contiguous() else vid.contiguous()
        if not torch.is_grad_enabled():
            return self.head_forward(text, vid_c.detach(), backward=False)["loss"][0].clone()
        return _HeadFn.apply(self, text, vid_c, *self._params())

    @torch.no_grad()
    def similarity(self, text_feat, vid_feat) -> torch.Tensor:
        """fp32 [B, B]: the L2-normalised, v_proj-projected, temperature-scaled matrix the loss sees (row i = text i, column j =
        video j; CSL_WDS: with its dual-softmax prior) -- the retrieval score.  Square batches only."""
        text, vid = self._inputs(text_feat, vid_feat)
        st = self.head_forward(text, (vid if vid.is_contiguous() else vid.contiguous()).detach(), backward=False, want_sim=True)
        return st["sim"].clone()


class TextEncoder:
    """Stand-in for model/TextEncoder.py (a frozen CLIP / BERT sentence encoder; the reference downloads it on construction).
    `.dim` sizes Matching.v_proj.  The encoder itself is whatever the user installs as `backend`: a callable from a list of
    caption strings to an fp32 [B, dim] tensor on the model's device -- or pass `text_feats=` to the model and never call this."""

    def __init__(self, enc_type, device=None, backend: Optional[Callable[[List[str]], torch.Tensor]] = None, dim: Optional[int] = None):
        """dim: the width of a user-supplied encoder when it is neither CLIP's 512 nor BERT's 768 (config key model.text_enc_dim)."""
        self.enc_type = enc_type
        self.device = device
        self.dim = int(dim) if dim is not None else (512 if str(enc_type).upper() == "CLIP" else 768)
        self.backend = backend

    def __call__(self, captions) -> torch.Tensor:
        if self.backend is None:
            raise RuntimeError("no text encoder is installed: pass text_feats= (fp32 [B, text_encoder.dim]) to the model / trainer, or "
                               "set model.text_encoder.backend to a callable mapping the captions to such a tensor")
        out = self.backend(captions)
        n = len(captions)
        if not torch.is_tensor(out) or out.dim() != 2 or tuple(out.shape) != (n, self.dim) or out.dtype != torch.float32:
            got = (tuple(out.shape), out.dtype) if torch.is_tensor(out) else type(out)
            raise ValueError(f"the text-encoder backend must return fp32 [{n}, {self.dim}], got {got}")
        return out
