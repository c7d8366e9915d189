"""Caption scores on the device: CIDEr-D rewards and SCST advantages (csrc/vct_cider.hip), BLEU / ROUGE-L / CIDEr for
evaluation (csrc/vct_capmetric.hip)."""
import torch

from .. import _lib as L


def _check_ids(ids, device, who, dims, tables):
    """The refusals of a candidate id table, before any launch: int64 of rank len(dims) on the GPU (on `device` when given), every
    extent >= 1 and at most 1 + VCT_CIDER_MAX_LEN columns (column 0 is the start token)."""
    if not torch.is_tensor(ids) or ids.dtype != torch.int64 or ids.dim() != len(dims):
        raise ValueError(f"{who}: ids must be an int64 tensor [{', '.join(dims)}], got {getattr(ids, 'dtype', type(ids))} "
                         f"{tuple(getattr(ids, 'shape', ()))}")
    if not ids.is_cuda or (device is not None and ids.device != device):
        raise ValueError(f"{who}: ids must live on the {tables} tables' device, got {ids.device}")
    if min(ids.shape) < 1 or ids.shape[-1] > 1 + L.CIDER_MAX_LEN:
        lead = "".join(f"{n} >= 1, " for n in dims[:-1])
        raise ValueError(f"{who}: ids [{lead}1 <= L <= {1 + L.CIDER_MAX_LEN}] (start column + at most {L.CIDER_MAX_LEN} tokens), "
                         f"got {tuple(ids.shape)}")


def check_cider_ids(ids, device=None):
    """The refusals of ops.cider_d's candidate table, before any launch: int64 [B, N, L] on the GPU (on `device` when given),
    1 <= L <= 1 + VCT_CIDER_MAX_LEN columns (column 0 is the start token)."""
    _check_ids(ids, device, "cider_d", ("B", "N", "L"), "reward")


def check_capmetric_ids(ids, device=None):
    """The refusals of the caption-metric kernels' candidate table, before any launch: int64 [C, L] on the GPU (on `device` when
    given), 1 <= L <= 1 + VCT_CIDER_MAX_LEN columns (column 0 is the start token)."""
    _check_ids(ids, device, "capmetric", ("C", "L"), "metric")


def _cider_desc(ids, shape, strides, vid_rows, tab):
    """vct_cider_desc of the [B, N, 1 + L] = `shape` view of `ids` with element `strides`; the reward pointer stays NULL."""
    d = L.CiderDesc()
    d.B, d.N, d.L, d.n = shape[0], shape[1], shape[2] - 1, int(tab.n)
    d.ids = ids.data_ptr()
    d.stride_b, d.stride_n, d.stride_l = strides
    d.end_id, d.log_nvid, d.two_sigma_sq = int(tab.end_id), float(tab.log_nvid), float(tab.two_sigma_sq)
    d.vid_rows, d.n_videos, d.table_cap = vid_rows.data_ptr(), int(tab.n_videos), int(tab.table_cap)
    for k in ("table_keys", "table_idf", "vid_ref_ptr", "ref_len", "ref_norm", "ref_ent_ptr", "ent_keys", "ent_w"):
        setattr(d, k, tab.t[k].data_ptr())
    return d


def cider_d(ids, vid_rows, tab, out=None):
    """CIDEr-D of sampled ids on the device (include/vct_hip.h, vct_cider_d).  ids: int64 [B, N, L] (any strides, column 0 the
    start token); vid_rows: int32 [B] table rows; tab: rewards.DeviceCiderD (its device tensors `t` and scalars); out: fp32
    [B, N] contiguous or None (allocated).  Returns out.  Enqueued on the current stream; no host synchronisation."""
    check_cider_ids(ids)
    B, N, Lc = ids.shape
    if vid_rows.dtype != torch.int32 or tuple(vid_rows.shape) != (B,) or not vid_rows.is_contiguous() or vid_rows.device != ids.device:
        raise ValueError(f"cider_d: vid_rows must be int32 [B = {B}] on {ids.device}, got {vid_rows.dtype} {tuple(vid_rows.shape)} on {vid_rows.device}")
    if not 1 <= int(tab.n) <= L.CIDER_MAX_ORDER:
        raise ValueError(f"cider_d: n-gram orders 1 .. {L.CIDER_MAX_ORDER}, got n = {tab.n}")
    if out is None:
        out = torch.empty(B, N, dtype=torch.float32, device=ids.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (B, N) or not out.is_contiguous() or out.device != ids.device:
        raise ValueError(f"cider_d: out must be contiguous fp32 [{B}, {N}] on {ids.device}, got {out.dtype} {tuple(out.shape)}")
    if tab.t["table_keys"].device != ids.device:
        raise ValueError(f"cider_d: the reward tables live on {tab.t['table_keys'].device}, ids on {ids.device}")
    d = _cider_desc(ids, (B, N, Lc), ids.stride(), vid_rows, tab)
    d.reward = out.data_ptr()
    L.check(L.load().vct_cider_d(d, L.stream_ptr()), "vct_cider_d")
    return out


def scst_advantages(rewards, baseline=None, adv=None, base_out=None, means=None):
    """Advantages of sampled captions on the device (include/vct_hip.h, vct_scst_advantages).  rewards: fp32 [B, N] contiguous;
    baseline: fp32 [B] (e.g. the greedy captions' rewards) or None = the leave-one-out mean of the video's other samples
    (needs N >= 2).  Returns (adv fp32 [B * N] in seq_w's layout, base_out fp32 [B], means fp32 [2] = mean reward, mean baseline);
    each may be passed in (adv may be rewards' own storage)."""
    if not torch.is_tensor(rewards) or rewards.dtype != torch.float32 or rewards.dim() != 2 or not rewards.is_cuda or not rewards.is_contiguous():
        raise ValueError(f"scst_advantages: rewards must be contiguous fp32 [B, N] on the GPU, got {getattr(rewards, 'dtype', type(rewards))} "
                         f"{tuple(getattr(rewards, 'shape', ()))}")
    B, N = rewards.shape
    if B < 1 or N < 1:
        raise ValueError(f"scst_advantages: rewards [B >= 1, N >= 1], got {tuple(rewards.shape)}")
    if baseline is None and N < 2:
        raise ValueError("scst_advantages: the leave-one-out baseline needs num_samples >= 2")

    def buf(x, shape, what):
        if x is None:
            return torch.empty(shape, dtype=torch.float32, device=rewards.device)
        if x.dtype != torch.float32 or x.numel() != shape[0] or not x.is_contiguous() or x.device != rewards.device:
            raise ValueError(f"scst_advantages: {what} must be contiguous fp32 with {shape[0]} elements on {rewards.device}, "
                             f"got {x.dtype} {tuple(x.shape)} on {x.device}")
        return x
    if baseline is not None:
        baseline = buf(baseline, (B,), "baseline")
    adv, base_out, means = buf(adv, (B * N,), "adv"), buf(base_out, (B,), "base_out"), buf(means, (2,), "means")
    L.check(L.load().vct_scst_advantages(B, N, rewards.data_ptr(), L.ptr(baseline), adv.data_ptr(), base_out.data_ptr(), means.data_ptr(),
                                         L.stream_ptr()), "vct_scst_advantages")
    return adv, base_out, means


def _capmetric_out(x, shape, dtype, dev, what):
    if x is None:
        return torch.empty(shape, dtype=dtype, device=dev)
    if x.dtype != dtype or tuple(x.shape) != tuple(shape) or not x.is_contiguous() or x.device != dev:
        raise ValueError(f"{what} must be contiguous {dtype} {list(shape)} on {dev}, got {x.dtype} {tuple(x.shape)} on {x.device}")
    return x


def _capmetric_rows(ids, vid_rows, what):
    Cn = ids.shape[0]
    if (not torch.is_tensor(vid_rows) or vid_rows.dtype != torch.int32 or tuple(vid_rows.shape) != (Cn,) or not vid_rows.is_contiguous()
            or vid_rows.device != ids.device):
        raise ValueError(f"{what}: vid_rows must be contiguous int32 [C = {Cn}] on {ids.device}, got "
                         f"{getattr(vid_rows, 'dtype', type(vid_rows))} {tuple(getattr(vid_rows, 'shape', ()))}")


def capmetric_counts(ids, vid_rows, tab, counts=None, rouge=None):
    """Per-caption BLEU / ROUGE-L statistics on the device (include/vct_hip.h, vct_capmetric_counts).  ids: int64 [C, L] (any
    strides, column 0 the start token); vid_rows: int32 [C] table rows; tab: metrics.DeviceCaptionMetrics (its device tensors `t`,
    end_id, beta_sq, n_videos); counts int32 [C, 12] / rouge fp64 [C, 3]: contiguous or None (allocated).  Returns (counts, rouge).
    Enqueued on the current stream; no host synchronisation."""
    check_capmetric_ids(ids)
    _capmetric_rows(ids, vid_rows, "capmetric_counts")
    Cn, Lc = ids.shape
    t = tab.t
    if t["ref_tok"].device != ids.device:
        raise ValueError(f"capmetric_counts: the metric tables live on {t['ref_tok'].device}, ids on {ids.device}")
    if not float(tab.beta_sq) > 0.0:
        raise ValueError(f"capmetric_counts: beta_sq > 0, got {tab.beta_sq}")
    counts = _capmetric_out(counts, (Cn, L.CAPMETRIC_COUNT_COLS), torch.int32, ids.device, "capmetric_counts: counts")
    rouge = _capmetric_out(rouge, (Cn, 3), torch.float64, ids.device, "capmetric_counts: rouge")
    d = L.CapMetricDesc()
    d.C, d.L = Cn, Lc - 1
    d.ids, d.stride_c, d.stride_l = ids.data_ptr(), ids.stride(0), ids.stride(1)
    d.end_id, d.vid_rows, d.n_videos, d.beta_sq = int(tab.end_id), vid_rows.data_ptr(), int(tab.n_videos), float(tab.beta_sq)
    for k in ("vid_ref_ptr", "ref_tok_ptr", "ref_tok"):
        setattr(d, k, t[k].data_ptr())
    d.counts, d.rouge = counts.data_ptr(), rouge.data_ptr()
    L.check(L.load().vct_capmetric_counts(d, L.stream_ptr()), "vct_capmetric_counts")
    return counts, rouge


def cider_d_eval(ids, vid_rows, tab, out=None):
    """The evaluation CIDEr of decoded ids on the device (include/vct_hip.h, vct_cider_d_eval): ops.cider_d's score with the end
    token dropped, un-rounded.  ids: int64 [C, L] (any strides); vid_rows: int32 [C]; tab: as ops.cider_d's (device tensors `t`
    and the scalars n, end_id, log_nvid, two_sigma_sq, n_videos, table_cap); out: fp64 [C] contiguous or None.  Returns out."""
    check_capmetric_ids(ids)
    _capmetric_rows(ids, vid_rows, "cider_d_eval")
    Cn, Lc = ids.shape
    if not 1 <= int(tab.n) <= L.CIDER_MAX_ORDER:
        raise ValueError(f"cider_d_eval: n-gram orders 1 .. {L.CIDER_MAX_ORDER}, got n = {tab.n}")
    if tab.t["table_keys"].device != ids.device:
        raise ValueError(f"cider_d_eval: the metric tables live on {tab.t['table_keys'].device}, ids on {ids.device}")
    out = _capmetric_out(out, (Cn,), torch.float64, ids.device, "cider_d_eval: out")
    d = _cider_desc(ids, (Cn, 1, Lc), (ids.stride(0), 0, ids.stride(1)), vid_rows, tab)
    L.check(L.load().vct_cider_d_eval(d, out.data_ptr(), L.stream_ptr()), "vct_cider_d_eval")
    return out


def capmetric_finish(counts, rouge, cider=None, out=None):
    """The corpus-level fold of the per-caption rows (include/vct_hip.h, vct_capmetric_finish).  counts int32 [C, 12], rouge fp64
    [C, 3], cider fp64 [C] or None; all contiguous on one GPU.  Returns out fp64 [8] = {Bleu_1..4, ROUGE_L, CIDEr, their sum with
    Bleu_4, C}.  Enqueued on the current stream; no host synchronisation."""
    if (not torch.is_tensor(counts) or counts.dtype != torch.int32 or counts.dim() != 2 or counts.shape[1] != L.CAPMETRIC_COUNT_COLS
            or not counts.is_cuda or not counts.is_contiguous() or counts.shape[0] < 1):
        raise ValueError(f"capmetric_finish: counts must be contiguous int32 [C >= 1, {L.CAPMETRIC_COUNT_COLS}] on the GPU, got "
                         f"{getattr(counts, 'dtype', type(counts))} {tuple(getattr(counts, 'shape', ()))}")
    Cn = counts.shape[0]
    if not torch.is_tensor(rouge):
        raise ValueError("capmetric_finish: rouge must be a tensor")
    _capmetric_out(rouge, (Cn, 3), torch.float64, counts.device, "capmetric_finish: rouge")
    if cider is not None:
        if not torch.is_tensor(cider):
            raise ValueError("capmetric_finish: cider must be a tensor or None")
        _capmetric_out(cider, (Cn,), torch.float64, counts.device, "capmetric_finish: cider")
    out = _capmetric_out(out, (8,), torch.float64, counts.device, "capmetric_finish: out")
    L.check(L.load().vct_capmetric_finish(Cn, counts.data_ptr(), rouge.data_ptr(), L.ptr(cider), out.data_ptr(), L.stream_ptr()),
            "vct_capmetric_finish")
    return out
