"""Greedy decoding (reference: model/MMT4Caption.py:146-184, model/CapDecoder.py:62-79).

Two implementations with identical results (tests/test_model_gpu.py):
  * `greedy_decode_ids_reference_algorithm`: the reference's O(L^2) loop -- every step re-runs the whole
    decoder over all tokens so far -- on the HIP kernels; one host sync per token like the reference's
    `.tolist()` (MMT4Caption.py:168).
  * `greedy_decode_ids` (default): KV cache (self-attention K/V per layer [B, Lmax, 2d], cross-attention
    K/V of the memory computed once), ONE new token per step, the per-token kernel sequence captured
    in a hipGraph per position and replayed; end-of-sequence bookkeeping stays on the device and the
    host reads it `lookahead` steps behind the launch front, so the device never idles on the check.
    The reference's stop rule (stop when EVERY row has emitted [SEP] at least once) is honoured by
    truncating the id matrix at that step.

Beam search (`beam_decode_ids`, `beam_decode_ids_reference_algorithm`): the reference has none (MMT4Caption.py:186 is a stub,
predict_video.py:170's `--beam` says "not support yet"); the semantics are stated in `beam_decode_ids`.

Sampling (`sample_decode_ids`, `sample_decode_ids_reference_algorithm`): temperature, top-k and nucleus draws, N captions
per video with their log-probabilities; the reference has none either, the semantics are stated in `sample_decode_ids`.

Generation controls (`GenerationControls`, `apply_controls_host`): minimum length, no-repeat n-gram ban, repetition penalty and
banned ids, applied to the step's logits on the device in front of the selection of all three decoders (`controls=`); the
reference has none, the semantics are stated in `GenerationControls`.

Ensembles (`Ensemble`): several models behind one greedy / beam / sampled session, their next-token distributions averaged on the
device at every step (decode/ensemble.py); the reference decodes with one checkpoint."""
from ..engine import memory_len
from .controls import (CONTROLS_BANNED_MAX, CONTROLS_MAX_LEN, CONTROLS_NGRAM_MAX, CONTROLS_THETA_MAX, GenerationControls, _f32,
                       _resolve_controls, apply_controls_host)
from .rules import (SAMPLE_TOP_K_MAX, _beam_finish, _beam_size, _check_sample_args, _draw_seed, _hash32, _no_beam_attn,
                    sample_uniforms)
from .cached import (_inputs_key, _run_session, _session, _token_loop, beam_decode_ids, greedy_decode_ids, sample_decode_ids,
                     teacher_forced_next_ids)
from .ensemble import ENSEMBLE_MAX, Ensemble, normalise_weights
from .reference import (_sample_select_ref, _select_ref, beam_decode_ids_reference_algorithm,
                        greedy_decode_ids_reference_algorithm, sample_decode_ids_reference_algorithm)
