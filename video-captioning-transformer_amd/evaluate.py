"""Inference-side callers of the caption path (reference eval.py:126-168, train.py:171-203).

`v2t_batch` / `v2t_single` keep the reference signatures (minus `local_args`: the device is the model's).  `eval_epoch`
decodes a whole split in batches and returns {video id: caption}; `val_epoch` is the teacher-forced validation loss
(train.py:150-167).  COCO scoring (eval.py:42-123) needs Java + pycocoevalcap, neither of which this image has:
`make_coco_sample` reshapes the dictionaries exactly as eval.py:24-39 does so that an external scorer can be fed, and
`score_coco` says why it cannot run here instead of pretending.  `eval_metrics` scores a split with the project's own BLEU-1..4,
ROUGE-L and CIDEr on the device (metrics.py; no METEOR) and `metric_earlystop_score` is the number metric early stopping watches."""
from typing import Dict, List, Optional, Sequence

import torch


def _strip_special(s: str) -> str:
    return s.replace("[CLS]", "").replace("[SEP]", "")          # eval.py:143, train.py:200


_SAMPLE_KEYS = ("num_samples", "temperature", "top_k", "top_p", "seed")


def _check_sample(sample, beam_size, return_attn):
    if sample is None:
        return
    if beam_size is not None or return_attn:
        raise ValueError("sample= excludes beam_size and return_attn: sampling is its own decoder and returns no attention maps")
    unknown = sorted(set(sample) - set(_SAMPLE_KEYS))
    if unknown:
        raise ValueError(f"sample= takes {_SAMPLE_KEYS}, got {unknown}")


@torch.no_grad()
def _decode(model, feats, masks, max_len, beam_size, return_attn=False, sample=None, controls=None):
    if sample is not None:
        return model.sample_decode(feats, masks, max_len=max_len, controls=controls, **sample)
    if beam_size is None:
        return model.greedy_decode(feats, masks, max_len=max_len, return_attn=return_attn, controls=controls)
    return model.beam_decode(feats, masks, beam_size=beam_size, max_len=max_len, return_attn=return_attn, controls=controls)


def average_attention(maps: torch.Tensor, length: Optional[int] = None) -> torch.Tensor:
    """The matrix predict_video.visualize plots (predict_video.py:126-142): the mean over layers of one caption's maps
    [layers, steps, Te] -> [steps, Te] (a batch [B, layers, steps, Te] -> [B, steps, Te]), cut to the first `length` generated
    tokens.  Plotting itself is left to the caller."""
    if maps.dim() not in (3, 4):
        raise ValueError("maps: [layers, steps, Te] of one caption or [B, layers, steps, Te]")
    avg = maps.float().mean(dim=maps.dim() - 3)
    return avg if length is None else avg[..., :int(length), :]


@torch.no_grad()
def v2t_batch(model, video_feats: Sequence[torch.Tensor], video_masks: Optional[Sequence[torch.Tensor]], max_len: int = 30,
              beam_size: Optional[int] = None, return_attn: bool = False, sample: Optional[dict] = None, controls=None):
    """eval.py:126-145: video_feats = list (one per modality) of [B, T, E]; masks = list of bool [B, T] or None.
    beam_size: None = greedy (the reference's only mode), else beam search with that many beams (MMT4Caption.beam_decode).
    return_attn (greedy only): (captions, cross-attention maps fp32 [B, layers, steps, Te]) -- MMT4Caption.greedy_decode_ids.
    sample = dict(num_samples=..., temperature=..., top_k=..., top_p=..., seed=...) (any subset): sampled decoding
    (MMT4Caption.sample_decode); returns for every video the list of its num_samples captions.  Excludes beam_size and
    return_attn (ValueError).  controls: a decode.GenerationControls (minimum length, no-repeat n-gram ban, repetition penalty,
    banned ids) for whichever decoder runs; combines with beam_size, sample and return_attn."""
    _check_sample(sample, beam_size, return_attn)
    model.eval()
    dev = model.device
    video_feats = [f.to(dev, non_blocking=True) for f in video_feats]
    video_masks = [m.to(dev, non_blocking=True) for m in video_masks] if video_masks is not None else None
    if return_attn:
        caps, maps = _decode(model, video_feats, video_masks, max_len, beam_size, True, controls=controls)
        return [_strip_special(r) for r in caps], maps
    if sample is not None:
        return [[_strip_special(r) for r in caps]
                for caps in _decode(model, video_feats, video_masks, max_len, None, sample=sample, controls=controls)]
    return [_strip_special(r) for r in _decode(model, video_feats, video_masks, max_len, beam_size, controls=controls)]


@torch.no_grad()
def v2t_frames(model, tower, videos: Sequence[torch.Tensor], max_len: int = 30, beam_size: Optional[int] = None,
               return_attn: bool = False, sample: Optional[dict] = None, extra_feats: Optional[Sequence[torch.Tensor]] = None,
               extra_masks: Optional[Sequence[torch.Tensor]] = None, controls=None):
    """predict_video.py --video, batched: videos = list of uint8 [T_i, H_i, W_i, 3] RGB frames (lengths and sizes may differ), tower =
    a vision.ClipVisionTower.  Each video is encoded on the device into its rows of ONE padded [B, max T_i, dim] matrix (padding
    rows zero, mask True there) and that goes to v2t_batch with its keywords: no feature visits the host.  A model with more than
    one feature stream takes the other streams' precomputed features as extra_feats (list of [B, T, E], in modal order behind the
    first) with extra_masks (list of bool [B, T], or None when nothing is padded).  controls: as v2t_batch."""
    _check_sample(sample, beam_size, return_attn)
    shapes = list(model.model_config["modal_shape"])
    if tower.dim != shapes[0]:
        raise ValueError(f"v2t_frames: the tower yields {tower.dim} features per frame, the model's first modal_shape entry is {shapes[0]}")
    extra_feats = list(extra_feats) if extra_feats is not None else []
    if len(extra_feats) != len(shapes) - 1:
        raise ValueError(f"v2t_frames: the model has {len(shapes)} feature streams; extra_feats must hold the other {len(shapes) - 1}, "
                         f"got {len(extra_feats)}")
    if len(videos) < 1 or any(not torch.is_tensor(v) or v.dim() != 4 or v.shape[0] < 1 for v in videos):
        raise ValueError("v2t_frames: videos is a non-empty list of uint8 [T, H, W, 3] tensors with T >= 1")
    if extra_masks is not None and len(extra_masks) != len(extra_feats):
        raise ValueError("v2t_frames: extra_masks must pair with extra_feats")
    dev = tower.device
    B, T = len(videos), max(v.shape[0] for v in videos)
    feats = torch.zeros(B, T, tower.dim, dtype=torch.float32, device=dev)
    lengths = torch.tensor([v.shape[0] for v in videos])
    for b, v in enumerate(videos):
        tower.encode_frames(v, out=feats[b, :v.shape[0]])
    mask = (torch.arange(T)[None, :] >= lengths[:, None]).to(dev, non_blocking=True)
    ragged = bool((lengths != T).any())
    masks = None
    if ragged or extra_masks is not None:
        others = list(extra_masks) if extra_masks is not None else [torch.zeros(f.shape[:2], dtype=torch.bool) for f in extra_feats]
        masks = [mask] + others
    return v2t_batch(model, [feats] + extra_feats, masks, max_len=max_len, beam_size=beam_size, return_attn=return_attn, sample=sample,
                     controls=controls)


@torch.no_grad()
def v2t_single(model, video_feat: Sequence[torch.Tensor], max_len: int = 30, beam_size: Optional[int] = None,
               return_attn: bool = False, sample: Optional[dict] = None, controls=None):
    """train.py:194-203: one video (list of [T, E] per modality), no mask.  return_attn: (caption, maps fp32 [layers, steps, Te]).
    sample (see v2t_batch): the list of the video's num_samples sampled captions.  controls: as v2t_batch."""
    _check_sample(sample, beam_size, return_attn)
    model.eval()
    feats = [f.unsqueeze(0).to(model.device) for f in video_feat]
    if return_attn:
        caps, maps = _decode(model, feats, None, max_len, beam_size, True, controls=controls)
        return _strip_special(caps[0]), maps[0]
    if sample is not None:
        return [_strip_special(r) for r in _decode(model, feats, None, max_len, None, sample=sample, controls=controls)[0]]
    return _strip_special(_decode(model, feats, None, max_len, beam_size, controls=controls)[0])


@torch.no_grad()
def eval_epoch(model, dataloader, max_len: int = 30, beam_size: Optional[int] = None, controls=None) -> Dict[str, str]:
    """train.py:171-180 / eval.py:156-160 without the scorer: captions for every video a by_video loader yields
    -> {vid: caption}.  Decoding is batched (the reference's eval config uses batch_size 1).  controls: as v2t_batch."""
    model.eval()
    vid2result: Dict[str, str] = {}
    for v_feats, v_masks, _caps, vids in dataloader:
        vid2result.update(zip(vids, v2t_batch(model, v_feats, v_masks, max_len=max_len, beam_size=beam_size, controls=controls)))
    return vid2result


@torch.no_grad()
def val_epoch(model, dataloader, mode: str = "caption", text_feats_fn=None, with_stats: bool = False):
    """train.py:150-167: mean loss over the loader, model in eval mode -- teacher-forced for 'caption' (a float), the contrastive
    loss for 'match' (a float), (loss, cap_loss, match_loss) for 'cross'.  text_feats_fn(captions, vids) -> fp32
    [B, text_encoder.dim] (match / cross); without it model.text_encoder(captions).  One device->host sync per epoch.
    With caption_decoder.label_smoothing > 0 the caption loss is the SMOOTHED criterion, as the reference's loop would return it.
    with_stats=True ('caption' / 'cross'): returns (that value, {"nll": ..., "token_acc": ...}) -- the epoch means (over batches, like
    the loss) of the un-smoothed NLL per token and of the token accuracy, read in the same single sync."""
    if mode not in ("caption", "match", "cross"):
        raise ValueError(f"unknown task {mode!r}")
    if with_stats and mode == "match":
        raise ValueError("with_stats: the match task has no caption loss")
    model.eval()
    model.mode(mode)
    model.check_task(mode)
    dev = model.device
    if with_stats:
        was = model.cap_decoder.loss_stats
        model.cap_decoder.loss_stats = True
        try:
            return _val_epoch(model, dataloader, mode, text_feats_fn, dev, True)
        finally:
            model.cap_decoder.loss_stats = was
    return _val_epoch(model, dataloader, mode, text_feats_fn, dev, False)


def _val_epoch(model, dataloader, mode, text_feats_fn, dev, with_stats):
    total, n = torch.zeros(3 if mode == "cross" else 1, device=dev), 0
    stats = torch.zeros(2, device=dev)
    for v_feats, v_masks, captions, vids in dataloader:
        v_feats = [f.to(dev, non_blocking=True) for f in v_feats]
        v_masks = [m.to(dev, non_blocking=True) for m in v_masks]
        if mode == "caption":
            total += model(v_feats, v_masks, captions).detach().reshape(1)
        else:
            text = text_feats_fn(captions, vids) if text_feats_fn is not None else model.text_encoder(captions)
            text = text.to(dev, non_blocking=True) if torch.is_tensor(text) else text
            out = model(v_feats, v_masks, captions, text_feats=text)
            total += torch.stack([o.detach() for o in out]) if mode == "cross" else out.detach().reshape(1)
        if with_stats:
            stats += model.cap_decoder._engine().last_loss_stats
        n += 1
    vals = torch.cat([total, stats]).tolist()
    out = tuple(v / max(n, 1) for v in vals[:-2]) if mode == "cross" else vals[0] / max(n, 1)
    if with_stats:
        return out, {"nll": vals[-2] / max(n, 1), "token_acc": vals[-1] / max(n, 1)}
    return out


def _reference_ids(pre, caption) -> List[int]:
    """A reference caption as the model's caption preprocessor tokenises it, start and end token stripped."""
    ids = pre.tokenizer.encode(caption) if isinstance(caption, str) else [int(t) for t in caption]
    if ids and ids[0] == pre.start_id:
        ids = ids[1:]
    if ids and ids[-1] == pre.end_id:
        ids = ids[:-1]
    return ids


def build_scorer(model, video2caption: Dict[str, List[str]], level: str = "token"):
    """The device scorer eval_metrics uses, over the references {vid: [caption, ...]} of one split; build it once and pass it as
    eval_metrics(scorer=...) every epoch.  level "token": ids of the model's tokenizer; "word": metrics.normalize_caption words
    through a metrics.WordTable (kept on the scorer as `.words`)."""
    from . import metrics
    if level == "token":
        pre = model.cap_preprocessor
        refs = {vid: [_reference_ids(pre, c) for c in caps] for vid, caps in video2caption.items()}
        scorer = metrics.CaptionMetrics(refs, end_id=pre.end_id).to_device(model.device)
        scorer.words = None
    elif level == "word":
        words = metrics.WordTable()
        refs = {vid: [words.encode(c) for c in caps] for vid, caps in video2caption.items()}
        scorer = metrics.CaptionMetrics(refs).to_device(model.device)
        scorer.words = words
    else:
        raise ValueError(f"level must be 'token' or 'word', got {level!r}")
    scorer.level = level
    return scorer


def _word_rows(scorer, captions: Sequence[str], device) -> torch.Tensor:
    """Captions -> the id matrix DeviceCaptionMetrics.add takes: column 0 a start column, the words' ids, then the end id."""
    rows = [scorer.words.encode(c) for c in captions]
    width = max(len(r) for r in rows)
    if width > 64:
        raise ValueError(f"eval_metrics: a caption of {width} words; the device scorer takes at most 64")
    host = torch.full((len(rows), 1 + max(width, 1)), scorer.end_id, dtype=torch.long)
    for i, r in enumerate(rows):
        host[i, 1:1 + len(r)] = torch.tensor(r, dtype=torch.long)
    return host.to(device)


@torch.no_grad()
def eval_metrics(model, dataloader, max_len: int = 30, beam_size: Optional[int] = None, level: str = "token", scorer=None,
                 return_captions: bool = False, controls=None):
    """train.py:171-192 / eval.py:156-168 with the scoring on the device: decodes every video a by_video loader yields (greedy, or
    beam search with beam_size beams; controls: a decode.GenerationControls for that decoder) and returns {Bleu_1..4, ROUGE_L, CIDEr, sum} (metrics.py), or (that, {vid: caption} exactly
    as eval_epoch returns it) with return_captions.

    level "token": the references are the loader's dataset.video2caption tokenised once by the model's caption preprocessor; the
    decoded id matrix goes straight into the scorer -- no string is built and no id leaves the device.  level "word": captions
    are decoded to strings and compared as metrics.normalize_caption words, the form coco-caption scores; use it when reporting
    numbers.  scorer: a build_scorer(model, video2caption, level) result to reuse the reference tables across epochs.
    Only videos with an entry in the references are scored and counted (an entry with an empty list scores 0 and counts);
    return_captions still returns every decoded video.

    The `sum` has THREE terms (Bleu_4 + ROUGE_L + CIDEr) where the reference's early-stopping sum adds METEOR as a fourth:
    METEOR needs Java and WordNet data and is not computed."""
    if level not in ("token", "word"):
        raise ValueError(f"level must be 'token' or 'word', got {level!r}")
    if not 2 <= int(max_len) <= 65:
        raise ValueError(f"eval_metrics: 2 <= max_len <= 65 (the device scorer takes at most 64 tokens after the start token), got {max_len}")
    dataset = getattr(dataloader, "dataset", None) or getattr(dataloader, "ds", None)      # torch's DataLoader / data.DeviceLoader
    if scorer is None:
        if dataset is None:
            raise ValueError("eval_metrics: the loader has no dataset to take references from; pass scorer=build_scorer(...)")
        scorer = build_scorer(model, dataset.video2caption, level)
    elif getattr(scorer, "level", level) != level:
        raise ValueError(f"eval_metrics: the scorer was built for level {scorer.level!r}, not {level!r}")
    model.eval()
    dev = model.device
    try:
        capacity = max(len(dataset), 1)
    except TypeError:
        capacity = 1024
    scorer.begin(capacity)
    vid2result: Dict[str, str] = {}
    for v_feats, v_masks, _caps, vids in dataloader:
        v_feats = [f.to(dev, non_blocking=True) for f in v_feats]
        v_masks = [m.to(dev, non_blocking=True) for m in v_masks] if v_masks is not None else None
        if beam_size is None:
            ys = model.greedy_decode_ids(v_feats, v_masks, max_len=max_len, controls=controls)
        else:
            ys = model.beam_decode_ids(v_feats, v_masks, beam_size=beam_size, max_len=max_len, controls=controls)
        caps = None
        if level == "word" or return_captions:
            caps = [_strip_special(c) for c in model._ids_to_captions(ys)]
            vid2result.update(zip(vids, caps))
        # a by_video loader walks the feature directory: clips the split holds no reference entry for are decoded, not scored
        known = [i for i, v in enumerate(vids) if v in scorer.vid_row]
        if not known:
            continue
        if level == "token":
            rows = ys if len(known) == len(vids) else ys.index_select(0, torch.tensor(known, device=ys.device))
        else:
            rows = _word_rows(scorer, [caps[i] for i in known], dev)
        scorer.add(rows, [vids[i] for i in known])
    out = scorer.result()
    return (out, vid2result) if return_captions else out


def metric_earlystop_score(metrics: dict) -> float:
    """The number metric early stopping watches (train.py:262-270: EarlyStopping(-sum of the metrics, ...)): metrics["sum"] =
    Bleu_4 + ROUGE_L + CIDEr.  Three terms where the reference's sum has four: METEOR is not computed here, so the values are not
    comparable with the reference's, only with each other."""
    return float(metrics["sum"])


@torch.no_grad()
def eval_retrieval(model, dataloader, text_feats_fn=None, mode: Optional[str] = None, tau=None) -> dict:
    """Text-video retrieval over the split a by_video loader walks (retrieval.py): embeds every batch's videos
    (MMT4Caption.embed_videos), takes the text features of EVERY reference caption of those videos (dataset.video2caption;
    text_feats_fn(captions, vids) -> fp32 [len(captions), text_encoder.dim] as in val_epoch, vids[k] the video of caption k, or the
    installed text_encoder.backend) and scores recall at 1 / 5 / 10, median and mean rank in both directions on the device.
    mode None: 'dual_softmax' with the head's temperature for a CSL_WDS head, 'plain' otherwise; tau overrides the temperature.
    A video without a reference entry is embedded and competes, but is no video->text query.  One device->host sync.
    Returns {"t2v": {R1, R5, R10, MedianR, MeanR, n}, "v2t": {...}, "rsum"}; recalls in percent."""
    from .retrieval import DeviceRetrievalMetrics
    model.check_task("match")
    dataset = getattr(dataloader, "dataset", None) or getattr(dataloader, "ds", None)
    v2c = getattr(dataset, "video2caption", None)
    if v2c is None:
        raise ValueError("eval_retrieval: the loader's dataset has no video2caption to take the reference captions from")
    if mode is None:
        mode = "dual_softmax" if model.matching.loss_fn.kind == "CSL_WDS" else "plain"
    if mode == "dual_softmax" and tau is None:
        tau = model.matching.loss_fn.temperature
        if tau is None:
            raise ValueError("eval_retrieval: mode 'dual_softmax' needs a tau: the head has no temperature, pass tau=")
        tau = tau.detach()
    model.eval()
    dev = model.device
    batches = []
    n_videos = n_texts = 0
    scorer = DeviceRetrievalMetrics(mode, tau, dev)
    # the scorer's matrices are sized once: embed first (device tensors, nothing is read back), then copy the rows in
    for v_feats, v_masks, _caps, vids in dataloader:
        v_feats = [f.to(dev, non_blocking=True) for f in v_feats]
        v_masks = [m.to(dev, non_blocking=True) for m in v_masks] if v_masks is not None else None
        emb = model.embed_videos(v_feats, v_masks)
        caps, cap_vids = [], []
        for v in vids:
            for c in v2c.get(v, ()):
                caps.append(c)
                cap_vids.append(v)
        text = None
        if caps:
            text = text_feats_fn(caps, cap_vids) if text_feats_fn is not None else model.text_encoder(caps)
            text = text.to(dev, non_blocking=True)
        batches.append((emb, list(vids), text, cap_vids))
        n_videos += len(vids)
        n_texts += len(caps)
    if not n_videos or not n_texts:
        raise ValueError(f"eval_retrieval: {n_videos} videos and {n_texts} reference captions: nothing to rank")
    scorer.begin(n_videos, n_texts)
    for emb, vids, text, cap_vids in batches:
        scorer.add_videos(emb, vids)
        if text is not None:
            scorer.add_texts(text, cap_vids)
    return scorer.result()


def retrieval_earlystop_score(metrics: dict) -> float:
    """The number retrieval early stopping watches: metrics["rsum"], the sum of the six recalls (use it as metric_earlystop_score)."""
    return float(metrics["rsum"])


def make_coco_sample(prediction_dict: Dict[str, str], ground_truth_dict: Dict[str, List[str]]):
    """eval.py:24-39: (gts, samples, IDs) in the layout COCOScorer.score expects."""
    samples, IDs, gts = {}, [], {}
    for vid, cap in prediction_dict.items():
        IDs.append(vid)
        samples[vid] = [{u"image_id": vid, u"caption": cap}]
    for vid, caps in ground_truth_dict.items():
        gts[vid] = [{u"image_id": vid, u"caption": cap} for cap in caps]
    return gts, samples, IDs


def score_coco(gts, samples, IDs):
    """BLEU/METEOR/ROUGE/CIDEr (eval.py:42-123) shell out to Java through pycocoevalcap.  Not available in this image."""
    try:
        from pycocoevalcap.bleu.bleu import Bleu      # noqa: F401
    except Exception as e:
        raise RuntimeError("COCO caption scoring needs pycocoevalcap + a Java runtime (reference submodule "
                           "submodules/pycocoevalcap); neither is installed here. Feed make_coco_sample()'s output to "
                           "the reference's COCOScorer on a machine that has them.") from e
    raise RuntimeError("pycocoevalcap found but scoring is not wired: use the reference's COCOScorer")
