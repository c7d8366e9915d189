"""Tensor-level wrappers over the C ABI (include/vct_hip.h).  PyTorch supplies device memory and the
current HIP stream; every function here enqueues hand-written gfx950 kernels and nothing else.

One module per kernel family; callers use `ops.X` and never import a submodule, so a function replaced on this
package (tests, tools/count_edges.py) is the one the engine, trainer and decode code call.  The imports below are
every name the package exposes."""
from .. import _lib as L        # ops.L.GemmAdam, ops.L.GEMM_GROUP_MAX: the engine and the trainer reach the mirror through here
from ._common import Drop
from .attention import attn_bwd, attn_fwd, attn_weights
from .clip import grad_clip_apply, grad_segments_table, grad_sqnorm, grad_sqnorm_scratch
from .decoding import (beam_reorder, beam_select, beam_select_workspace_bytes, decode_block, decode_block_supported, decode_gemv,
                       decode_linear, decode_ln2, ensemble_combine, greedy_select, logit_controls, sample_select,
                       sample_select_workspace_bytes)
from .elementwise import advance_seed, argmax_rows, axpby, cast, gather_pad_rows, scale, transpose, warm
from .embed import embed_bwd, embed_fwd, embed_live_rebuild, embed_live_table, text_pool
from .frontend import (enc_frontend_bwd, enc_frontend_ex_bwd, enc_frontend_ex_fwd, enc_frontend_fwd, hmm_mix_bwd, hmm_mix_fwd,
                       mm_frontend_bwd, mm_frontend_fwd)
from .gemms import GemmScratch, _gemm_desc, gemm, gemm_grouped, gemm_last_route, gemm_workspace_bytes
from .layer_ss import (SS_CHUNK, layer_ss_bwd, layer_ss_bwd_desc, layer_ss_bwd_stream_chunks, layer_ss_desc, layer_ss_fwd,
                       layer_ss_stream_chunks, layer_ss_supported, ss_pack)
from .loss import group_sum, sce_loss, sce_loss_ls, wce_loss
from .matching import match_agg_bwd, match_agg_fwd, match_loss, match_loss_workspace_bytes, retrieval_ranks, retrieval_workspace_bytes
from .norm import add_ln_bwd, add_ln_fwd, add_ln_ln_bwd, add_ln_ln_fwd, ln_param_finalize_batched, ln_ws_rows, preln_fwd
from .optim import adam_bump, adam_ranges_table, adam_step, adam_step_2d, adam_step_ranges
from .runtime import (TAPS, LaunchList, host_call, is_recording, masked_stream, stream_wait, sync_record, sync_wait, tap,
                      tap_collect, taps_enable)
from .scoring import capmetric_counts, capmetric_finish, check_capmetric_ids, check_cider_ids, cider_d, cider_d_eval, scst_advantages
from .vision import frames_to_patches, vit_embed, vit_pool
