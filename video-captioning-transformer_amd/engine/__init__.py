"""Forward / backward schedules of the caption path over the gfx950 kernels.

The reference runs this path as ~60 stock torch.nn calls under autograd (model/MMEncoder.py:244-276,
model/CapDecoder.py:34-60, torch nn/modules/transformer.py:951-982,1143-1199).  Here the graph is
static and known, so forward and backward are explicit kernel schedules over pre-allocated HBM
buffers: no autograd tape, no temporaries, no host synchronisation -- the whole step is
hipGraph-capturable.  Every arithmetic step is a libvct_hip.so kernel (the ops package); torch is used for
memory, streams and a few boolean mask preparations only.

Data layout in HBM (row-major, tokens x features):
  encoder tokens   Me = B*(T+1) rows, decoder tokens Md = B*(S-1) rows, d columns
  packed projections qkv [M,3d], cross kv [Me,2d]; FFN hidden [M,ff]; logits [Md, Vp] with
  Vp = V rounded up to 32 and zero-padded columns; statistics (mean, rstd) fp32 [M].
  Activations are bf16 (throughput mode) or fp32 (parity mode); parameters stay fp32 masters with a
  bf16 shadow refreshed once per step; every parameter gradient is fp32.
"""
from .inputs import first_input, memory_len, stage_inputs, static_inputs
from .params import ParamSet, StepContext, _Buf
from .stack import DEC_SITE, DMEM_SYNC, EMB_SITE, ENC_IN_SITE, ENC_SITE, SAMPLE_SITE, _CUS, _StackBase, _cu_count
from .encoder import EncoderEngine, HMMEncoderEngine
from .decode_step import (BeamDecodeState, DecodeState, SampleDecodeState, _decoder_block_decode_ok, _decoder_decode_step,
                          _decoder_decode_step_any, _decoder_decode_step_block, _decoder_decode_step_fused, _decoder_decode_step_small,
                          _decoder_fused_decode_ok, _decoder_small_decode_ok, decode_step_variant)
from .decoder import DecoderEngine
