"""What the cached decoders and the reference algorithms share: the argument checks of beam search and sampling, the final
ranking of the beams, and the sampling seed with its counter hash."""
import math

import torch

from ..engine import SAMPLE_SITE


def _beam_size(beam_size, V: int) -> int:
    K = int(beam_size)
    if not 1 <= K <= 16 or K > V:
        raise ValueError(f"beam_size must be in 1..16 and <= the vocabulary size, got {beam_size}")
    return K


def _no_beam_attn(return_attn: bool):
    if return_attn:
        raise ValueError("return_attn is not supported by beam search: the maps would have to follow the beams' parent "
                         "back-track; use greedy_decode_ids(return_attn=True)")


def _beam_finish(ids: torch.Tensor, scores: torch.Tensor, B: int, K: int, end_id: int, length_penalty: float, return_all: bool):
    """ids [B*K, L'] (slot order), raw scores fp32 [B*K] -> the slots of each video sorted by s / n^alpha (descending, ties to
    the lower slot), n = generated tokens up to and including the first end_id (all of them if none)."""
    gen = ids[:, 1:] == end_id
    n_all = ids.shape[1] - 1
    first = torch.where(gen.any(1), gen.int().argmax(1) + 1, torch.full_like(gen[:, 0], n_all, dtype=torch.long))
    final = scores.float() / first.float().pow(float(length_penalty))
    final = final.view(B, K)
    final, order = torch.sort(final, dim=1, descending=True, stable=True)
    ids = ids.view(B, K, -1).gather(1, order[:, :, None].expand(-1, -1, ids.shape[1]))
    if return_all:
        return ids, final
    return ids[:, 0].contiguous()


# ---- sampling ------------------------------------------------------------------------------------------------------------------
SAMPLE_TOP_K_MAX = 64


def _check_sample_args(num_samples, temperature, top_k, top_p):
    """The range checks of sampled decoding: ValueError before any device work."""
    if int(num_samples) != num_samples or int(num_samples) < 1:
        raise ValueError(f"num_samples must be an integer >= 1, got {num_samples}")
    t = float(temperature)
    if not math.isfinite(t) or t <= 0.0:
        raise ValueError(f"temperature must be finite and > 0, got {temperature}")
    if int(top_k) != top_k or not 0 <= int(top_k) <= SAMPLE_TOP_K_MAX:
        raise ValueError(f"top_k must be in 0..{SAMPLE_TOP_K_MAX} (0 = the whole vocabulary), got {top_k}")
    p = float(top_p)
    if not (0.0 < p <= 1.0):
        raise ValueError(f"top_p must be in (0, 1], got {top_p}")
    if p < 1.0 and int(top_k) == 0:
        raise ValueError("top_p < 1 needs top_k >= 1: the nucleus is taken within the top-k candidates (a nucleus over the whole "
                         "vocabulary is not implemented and is not approximated silently); pass top_k (at most 64)")


def _draw_seed(seed) -> int:
    """seed=None: one draw from torch's default generator (torch.manual_seed makes a run reproducible); else as given."""
    if seed is None:
        return int(torch.randint(0, 2 ** 31 - 1, (1,)).item())
    return int(seed) & 0xFFFFFFFF


def _hash32(x: int) -> int:
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & 0xFFFFFFFF
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & 0xFFFFFFFF
    return x ^ (x >> 16)


def sample_uniforms(seed: int, rows: int, t: int):
    """The uniforms of step t for rows 0 .. rows-1 (csrc/vct_sample.hip, smp_uniform): the dropout kernels' counter hash at
    site SAMPLE_SITE, 24 bits each, as Python floats (exact)."""
    key = (((seed & 0xFFFFFFFF) * 0x9E3779B1) & 0xFFFFFFFF) ^ ((SAMPLE_SITE * 0x85EBCA77 + 0x165667B1) & 0xFFFFFFFF)
    k = _hash32(key)
    return [(_hash32((k + ((t * rows + r) & 0xFFFFFFFF) * 0x9E3779B1) & 0xFFFFFFFF) >> 8) / 16777216.0 for r in range(rows)]
