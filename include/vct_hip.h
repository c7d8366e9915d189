/*
 * vct_hip.h -- C ABI of libvct_hip.so: the MI355X (gfx950 / CDNA4) kernels behind the
 * video-caption Transformer training / greedy-decode path.
 *
 * The reference (Kamino666/Video-Captioning-Transformer) has no FFI for this path: every FLOP is a
 * stock torch.nn module call.  Each entry point below therefore cites the reference call site
 * (file:line under /root/reference) and the torch operator whose arithmetic it replaces.  A
 * reference maintainer binds them with ctypes; nothing here knows about torch.
 *
 * Conventions
 *  - every function returns int: 0 ok, <0 argument/shape error (VCT_E_*), >0 a hipError_t;
 *    nothing throws, nothing allocates, nothing synchronises the host: all work is enqueued on the
 *    caller's `stream` (a hipStream_t passed as void*), so every call is hipGraph-capturable.
 *  - all pointers are DEVICE pointers owned by the caller; tensors are row-major; "ld*" are leading
 *    dimensions in ELEMENTS.  Activations are VCT_F32 or VCT_BF16 ("compute dtype"); statistics,
 *    biases, LayerNorm parameters, losses and every parameter gradient are fp32.
 *  - leading dimensions of VCT_BF16 matrices must be multiples of 8 elements and base pointers
 *    16-byte aligned (VCT_F32: multiples of 4).  A K extent that is not a multiple of 8 (4) along a
 *    contiguous dimension must be zero-padded up to it by the producer (the SCE-loss kernel does
 *    this for the vocabulary dimension).
 *  - dropout: mask(site, idx) = hash(seed[0], site, idx) >= p * 2^32, scaled by 1/(1-p); `seed` is
 *    a DEVICE pointer (so a captured graph sees a new seed each replay); p == 0 or seed == NULL
 *    disables it.  The backward kernels recompute the same mask from (site, idx).
 */
#ifndef VCT_HIP_H
#define VCT_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VCT_ABI_VERSION 16

enum { VCT_F32 = 0, VCT_BF16 = 1 };
enum { VCT_ACT_NONE = 0, VCT_ACT_GELU = 1, VCT_ACT_RELU = 2,
       VCT_ACT_QUICK_GELU = 3 /* x * sigmoid(1.702 x), CLIP's activation.  vct_gemm's forward form only (ta = 0, tb = 1, no dact_src;
                                 anything else is VCT_E_ARG): it is compiled into no other kernel, and the `act` fields of the other
                                 descriptors (layer, decode) take NONE / GELU / RELU as before */ };
enum {
  VCT_OK = 0,
  VCT_E_ARG = -1,      /* null pointer / bad enum */
  VCT_E_SHAPE = -2,    /* unsupported or inconsistent shape */
  VCT_E_ALIGN = -3,    /* leading dimension / pointer alignment */
  VCT_E_WORKSPACE = -4 /* workspace too small */
};

int vct_abi_version(void);
/* writes "gfx950 ..." build string; returns its length */
int vct_build_info(char* buf, int buflen);

/* ---------------------------------------------------------------------------------------------
 * GEMM family: C[M,N] = epilogue(op(A)[M,K] * op(B)[K,N])   -- MFMA (bf16 16x16x32 / f32 16x16x4)
 *   ta == 0: A stored [M,K] (K contiguous)      ta == 1: A stored [K,M] (M contiguous)
 *   tb == 1: B stored [N,K] (nn.Linear weight)  tb == 0: B stored [K,N] (N contiguous)
 * replaces: nn.Linear forward (MMEncoder.py:246, CapDecoder.py:55, the linear1/linear2/in_proj/out_proj
 * inside nn.Transformer{En,De}coderLayer -- torch nn/modules/transformer.py:951-982,1143-1199 and
 * nn/functional.py:5785,6637) and its autograd backward (dX = dY*W: ta=0,tb=0; dW = dY^T*X: ta=1,tb=0).
 * --------------------------------------------------------------------------------------------- */
/* Optional OPTIMIZER epilogue of the weight-gradient form (dtype bf16, out fp32, ta=1, tb=0; vct_gemm and vct_gemm_grouped): the
 * gradient element g the product would store to C[r, c] is consumed in the epilogue registers by torch.optim.Adam's update of the
 * parameter element it belongs to,
 *     m += (1-b1)(g-m);  v = b2 v + (1-b2) g^2;  p = p (1 - lr wd) - (lr / (1 - b1^t)) m / (sqrt(v) / sqrt(1 - b2^t) + eps)
 * (exactly vct_adam_step's arithmetic; t = *step + 1, hyper = {lr, beta1, beta2, eps, weight_decay} in DEVICE memory), and the
 * refreshed bf16 shadow / stream-order packed copy of the weight are written from the same registers.
 * replaces: `optimizer.step()` of the reference (train.py:24-26,126: torch.optim.Adam over the weight) for THIS matrix, and the
 * 4 B / parameter gradient store + re-load between `loss.backward()` (train.py:125) and it -- the optimizer's HBM pass over the
 * matrix runs inside the MFMA-bound product that produced its gradient instead of as a serial tail of the step.
 *   param / exp_avg / exp_avg_sq: fp32 [M, ldc] -- element (r, c) at r * ldc + c, the layout of C (views of flat buffers at C's offset).
 *   shadow: bf16 [M, ld_shadow] or NULL.  pk_*: the matrix's stream-order packed copy as in vct_adam_pack_seg (K = row length of the
 *   WHOLE weight, pk_row0 = row of the whole weight that C's row 0 is, pk_stream NULL = none).
 *   store_grad != 0: C is written as well (tests, gradient hooks); 0: C is left untouched.
 * Single GPU only: a data-parallel exchange has to average g first (trainer.ShardedExchange keeps the separate pass). */
typedef struct vct_gemm_adam {
  float* param; float* exp_avg; float* exp_avg_sq;
  void* shadow; int64_t ld_shadow;
  void* pk_stream; int32_t pk_K, pk_mode; int32_t pk_chunk0[4]; int32_t pk_row0; int32_t store_grad;
  const float* hyper; const int32_t* step;
} vct_gemm_adam;

typedef struct vct_gemm_desc {
  int32_t dtype;      /* VCT_F32 | VCT_BF16 : element type of A and B */
  int32_t out_dtype;  /* element type of C, preact, addend */
  int32_t ta, tb;
  int32_t M, N, K;
  int32_t act;        /* VCT_ACT_*: applied after bias */
  const void* A; int64_t lda;
  const void* B; int64_t ldb;
  void* C; int64_t ldc;
  const float* bias;                        /* [N] or NULL */
  void* preact; int64_t ld_preact;          /* optional: acc+bias before act (saved for backward) */
  const void* addend; int64_t ld_addend;    /* optional: C += addend (residual-gradient accumulate) */
  const void* dact_src; int64_t ld_dact;    /* optional: C = acc * act'(dact_src) (type = out_dtype) */
  const uint32_t* seed; uint32_t site; float p_drop; /* dropout on C (after act / inside dact) */
  float* bias_grad;                         /* optional [M] fp32: sum over K of op(A) (db for ta=1) */
  void* workspace; int64_t workspace_bytes; /* split-K partials (fp32); NULL = never split */
  int32_t split_k;                          /* 0 auto, 1 none, >1 forced.  A forced split that cannot be honoured is REFUSED with
                                               VCT_E_WORKSPACE, never quietly dropped: no / too small a workspace, or a product with
                                               an epilogue (bias, act, preact, addend, dact_src, dropout, adam) that cannot reduce
                                               inside the kernel -- no tile_counters, fp32 operands, or more than 16 MB of fp32
                                               partials (split * M * N * 4).  The automatic split (0) falls back to no split there;
                                               a plain product falls back to the two-pass reduce. */
  int32_t reserved;                         /* 0; kernel-selection override for tests / A-B probes: 1-9 (+10 x buffers) = a tile of
                                               the general kernel, 100 = force / 99 = forbid the persistent-tile layer kernel;
                                               vct_gemm_last_route (below) reports the kernel that was actually launched */
  int32_t n_tile_counters;                  /* ints available at tile_counters */
  int32_t* tile_counters;                   /* optional, see below */
  const vct_gemm_adam* adam;                /* optional (NULL = none): optimizer epilogue of the dW form, see vct_gemm_adam */
} vct_gemm_desc;
/* tile_counters: device ints that are ZERO on entry (they are zero again when the GEMM has finished, so one
 * zero-filled allocation serves every later call on the same stream).  With them a split-K GEMM reduces inside
 * the producing kernel -- the last workgroup to finish a tile sums the partials in fixed split order
 * (bit-reproducible) -- instead of in a second launch.  Needs one int per output tile (<= M*N/4096 + M/64 + N/64
 * + 1 is always enough); without (NULL / too few) the two-pass reduce is used.  GEMMs that may run CONCURRENTLY
 * (different streams) must not share counters or workspace. */
int vct_gemm(const vct_gemm_desc* d, void* stream);
/* The route the calling thread's last vct_gemm / vct_gemm_grouped took: which kernel was launched, with which tile and split.  A
 * host-side, thread-local record written where the launch is issued (read-only here; all zero before the first GEMM of the thread;
 * a call that returned an error leaves it unspecified).  Tests assert it, so that a case written for one kernel cannot fall through
 * to another unnoticed when an eligibility threshold moves (`reserved` above forces a route, this reports the one taken).
 * out[0 .. VCT_GEMM_ROUTE_INTS):
 *   [0] kernel: 1 general bf16, 2 general fp32, 3 skinny, 4 persistent 256 x 256 (round-5 kernel), 5 persistent 256 x 256
 *       (pipelined g32 kernel), 6 persistent-tile layer kernel, 7 grouped
 *   [1] bm  [2] bn  (tile; skinny: 16 x 16 ntl)   [3] nbuf (operand stages; 0: no LDS staging)
 *   [4] variant: the general / grouped kernel's eight-wave variant id (0 four waves, 1 128x128, 4 128x64, 6 256x128, 7 320x128,
 *       9 64x128); skinny: ntl; layer kernel: 1 = the epilogue instantiation, 0 = the plain one
 *   [5] split (grouped: the largest of the problems)   [6] 1 = the split was reduced inside the producing kernel (tile counters)
 *   [7] 1 = a separate reduce launch followed
 *   [8] grouped: number of problems   [9 .. 9 + VCT_GEMM_GROUP_MAX) grouped: each problem's split
 * Returns VCT_E_ARG when out is NULL or n < VCT_GEMM_ROUTE_INTS. */
#define VCT_GEMM_ROUTE_INTS 17
int vct_gemm_last_route(int32_t* out, int32_t n);
/* bytes of workspace vct_gemm may use for this descriptor (0 if it will not split) */
int64_t vct_gemm_workspace_bytes(const vct_gemm_desc* d);

/* n (<= VCT_GEMM_GROUP_MAX) independent weight-gradient GEMMs in ONE launch: every descriptor must be the dW form
 * (dtype bf16, out fp32, ta=1, tb=0, no epilogue other than bias_grad).  replaces: the per-Linear
 * `grad_weight = grad_out.t() @ input` / `grad_bias = grad_out.sum(0)` autograd nodes of one Transformer layer
 * (torch autograd of F.linear as used by nn.TransformerEncoderLayer / DecoderLayer, MMEncoder.py:236,
 * CapDecoder.py:18), which the reference runs as 8-14 separate kernels per layer.
 * Each descriptor carries its OWN workspace (vct_gemm_grouped_workspace_bytes(descs, n, i) bytes) and its OWN
 * tile_counters (required whenever that is non-zero); split_k: 0 auto, >=1 forced. */
#define VCT_GEMM_GROUP_MAX 8
int vct_gemm_grouped(const vct_gemm_desc* descs, int32_t n, void* stream);
int64_t vct_gemm_grouped_workspace_bytes(const vct_gemm_desc* descs, int32_t n, int32_t i);

/* ---------------------------------------------------------------------------------------------
 * Multi-head attention core: O = softmax(Q K^T / sqrt(hd) + mask) V per (batch, head), one wave each,
 * QK^T and PV as MFMA tiles, K/V staged in LDS, row softmax by wave shuffles, dropout on P.
 * replaces: F.scaled_dot_product_attention + mask merge inside nn.MultiheadAttention
 * (torch nn/functional.py:6553-6570,6629) as used at MMEncoder.py:274, CapDecoder.py:49-52,70-75.
 *   q: rows b*Lq+i, cols h*hd..; k,v: rows b*Lk+j.  ld in elements.  causal: key j > query i masked.
 *   key_pad: uint8 / bool [B, Lk - key_pad_shift], 1 = padded key (masked) or NULL; the first key_pad_shift keys are never
 *   padded (the encoder passes the raw frame mask [B,T] with shift 1: key 0 is the aggregation token, MMEncoder.py:252-257).
 *   key_ids: alternative to key_pad -- int64 token ids, key j of batch b is padded iff key_ids[b*key_ids_bs + j] == pad_id
 *   (the decoder passes its id matrix: tgt_padding_mask[:, :-1] of CapDecoder.py:45-47 without materialising it).
 *   Limits: Lq, Lk <= 64, hd <= 128.
 * --------------------------------------------------------------------------------------------- */
typedef struct vct_attn_desc {
  int32_t dtype;
  int32_t B, H, Lq, Lk, hd;
  int32_t causal;
  int32_t key_pad_shift;
  const void* q; int64_t ldq;
  const void* k; int64_t ldk;
  const void* v; int64_t ldv;
  void* o; int64_t ldo;
  const uint8_t* key_pad;
  const uint32_t* seed; uint32_t site; float p_drop;
  /* backward only */
  const void* d_o; int64_t ld_do;
  void* dq; int64_t ld_dq;
  void* dk; int64_t ld_dk;
  void* dv; int64_t ld_dv;
  /* optional batch strides in ELEMENTS (0 = dense: L * ld).  A KV cache [B, Lmax, ...] read with
   * Lk < Lmax sets k_bs = v_bs = Lmax * ld. */
  int64_t q_bs, k_bs, v_bs, o_bs;
  const int64_t* key_ids; int64_t key_ids_bs; int64_t pad_id;
} vct_attn_desc;
int vct_attn_fwd(const vct_attn_desc* d, void* stream);
int vct_attn_bwd(const vct_attn_desc* d, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Head-averaged attention map: W[b, i, j] = (1/H) * sum_h softmax_j(q[b,i,h] . k[b,j,h] / sqrt(hd) + mask)[j], fp32 [B, Lq, Lk].
 * One wave per (batch, 16-query tile) walks the heads in ascending order and sums the probabilities in fp32 registers (no atomics,
 * no second pass: two runs are bitwise equal); scores, masks and exponentials are the forward's (csrc/vct_attn_core.h), so a map
 * is the probability vct_attn_fwd multiplied V with at p_drop = 0.  A fully masked row is all zero.  No V, no dropout, no O.
 * replaces: nn.MultiheadAttention's need_weights=True, average_attn_weights=True return value (torch nn/functional.py:6572-6589)
 * as VisTransformerDecoderLayer keeps it (CapDecoder.py:112-113) and as predict_video.py's patched layers record it per generated
 * token (predict_video.py:63-64).
 *   q, k, masks, dtype, limits and alignment: as vct_attn_desc (Lq, Lk <= 64, hd <= 128; q and k 16-byte aligned).
 *   w: fp32, row i of batch b at w + b * w_bs + i * ldw (ldw >= Lk; w_bs 0 = dense: Lq * ldw) -- a decode step writes row t-1 of a
 *   [B, layers, Lmax-1, Te] buffer with Lq = 1, w_bs = layers * (Lmax-1) * Te.
 * --------------------------------------------------------------------------------------------- */
typedef struct vct_attn_weights_desc {
  int32_t dtype;
  int32_t B, H, Lq, Lk, hd;
  int32_t causal;
  int32_t key_pad_shift;
  const void* q; int64_t ldq;
  const void* k; int64_t ldk;
  float* w; int64_t ldw;
  const uint8_t* key_pad;
  int64_t q_bs, k_bs, w_bs;          /* batch strides in ELEMENTS (0 = dense) */
  const int64_t* key_ids; int64_t key_ids_bs; int64_t pad_id;
} vct_attn_weights_desc;
int vct_attn_weights(const vct_attn_weights_desc* d, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Sample-stationary Transformer stack forward (bf16): ONE launch = up to 4 whole encoder / decoder layers (and, with last != 0
 * in the last descriptor, the stack-final LayerNorm); one 512-thread workgroup per SAMPLE keeps that sample's rows in LDS
 * from the first layer's input to the last layer's output and streams the weights from L2 straight into MFMA operand
 * registers (csrc/vct_layer_ss.hip).  layers[0 .. n_layers): one descriptor per layer, identical in shape, masks, memory, seed
 * and p_drop; layers[0].x is the stack input (the other x fields are ignored: a layer reads its predecessor's output from
 * LDS); the packed weight streams lie back to back (layers[l].wpk = layers[0].wpk + l * nchunks * 64 KiB).
 * replaces: nn.TransformerEncoderLayer.forward (torch nn/modules/transformer.py:951-982) / nn.TransformerDecoderLayer.forward
 * (:1143-1199) as built at MMEncoder.py:236-238 / CapDecoder.py:18-20 and run by MMEncoder.py:274 / CapDecoder.py:49-52
 * (post-norm, gelu / relu, eps 1e-5; nn.MultiheadAttention = torch nn/functional.py:6206-6640), plus the final
 * nn.LayerNorm of the stack (MMEncoder.py:238, CapDecoder.py:20) -- i.e. the vct_gemm / vct_attn_fwd / vct_add_ln_fwd /
 * vct_add_ln_ln_fwd launches of one layer on the unfused path.  It SAVES exactly what those save (qkv, o, a, y, mean, rstd,
 * cross q / kv / o / a, pre-activation, dropped activation, f) and draws the same dropout counter streams
 * (site_*: attention probabilities, residual dropouts, feed-forward dropout), so the unfused backward kernels run behind it.
 *   x bf16 [B*L, 512] layer input (an OUTPUT when layers[0].pro != 0: the rows the prologue builds); mem bf16 [B*Lm, 512] (decoder layers; NULL = encoder layer: no cross-attention block,
 *   n2 unused).  Self-attention masks as vct_attn_desc (causal; key_pad + key_pad_shift; key_ids / pad_id).
 *   wpk: the layer's weights packed in STREAM ORDER by vct_ss_pack -- 64-KiB chunks (one 512-row block x 64 K columns of a
 *   weight, as 8 waves x 8 MFMA fragments of 1 KiB: wave w, column tile t < 4, k-step s < 2 = rows 64w + 16t .. +15,
 *   columns 32s .. 32s + 31 of the chunk), blocks in consumption order:
 *     in_proj rows [0,512) [512,1024) [1024,1536) | out_proj | (decoder: cross in_proj rows [0,512) | [512,1024) [1024,1536) |
 *     cross out_proj) | linear1 rows [0,512) | for j < ff/512: linear1 rows [512(j+1), 512(j+2)) (while j+1 < ff/512) ,
 *     linear2 columns [512j, 512j+512)        (the feed-forward block is software-pipelined: the GELU / dropout of chunk j is
 *     issued between the K steps of linear1's block j+1)
 *   each block 8 chunks (K = 512); nchunks = vct_layer_ss_stream_chunks(ff, cross).
 *   The feed-forward activation is built on the pre-activation as stored (bf16), which is also what the backward's GELU' reads.
 * vct_layer_ss_supported: bf16, d = 512, 8 heads of 64, ff a multiple of 512 and <= 2048, L <= 32, Lm <= 16 (Lm = 0: encoder layer).
 * vct_ss_pack: segs[i] = rows 0..511 x columns 0..64*nchunks-1 of the bf16 matrix at `w` (leading dimension ldw; the caller
 *   offsets `w` to the block) -> chunks dst_chunk .. dst_chunk+nchunks-1 of `dst`.  One launch per 48 segments.
 * --------------------------------------------------------------------------------------------- */
typedef struct vct_ss_norm { const float* gamma; const float* beta; void* y; float* mean; float* rstd; } vct_ss_norm;
typedef struct vct_layer_ss_desc {
  int32_t dtype, B, L, Lm, d, H, ff, act;
  int32_t last, causal, key_pad_shift, reserved;
  const void* wpk; int64_t nchunks;
  const void* x; const void* mem;
  const float* b_qkv; const float* b_o;
  void* qkv; void* o; void* a;
  vct_ss_norm n1;
  const float* b_cq; const float* b_ckv; const float* b_co;
  void* cq; void* ckv; void* co; void* ca;
  vct_ss_norm n2;
  const float* b1; const float* b2;
  void* hpre; void* h; void* f;
  vct_ss_norm n3;
  vct_ss_norm nf;
  const uint8_t* key_pad; const int64_t* key_ids; int64_t key_ids_bs; int64_t pad_id;
  const uint32_t* seed; float p_drop;
  uint32_t site_sa, site_n1, site_ca, site_n2, site_ff, site_n3;
  uint32_t site_emb;
  /* stack prologue (layers[0] only): pro = 0: x is the input.  pro = 1 (encoder stacks): x is BUILT from the frame features --
   * u = feats W_u^T + b_unify (the unify weight's 512 x 512 block = the FIRST 8 chunks of the stream, in front of layer 0's),
   * row 0 = mean_t(u) + pe_rows[0], row t+1 = u_t + pe_rows[t+1] (MMEncoder.py:246-271) -- stored to x, and the bf16 copy of fp32
   * features to x_in (what the unify weight gradient reads; NULL when feats are bf16).  pro = 2 (decoder stacks): x = dropout(
   * emb_table[emb_ids[b, s]] + emb_pos[s]) (CapDecoder.py:48, Embedding.py:23-25; counter stream of vct_embed_fwd, site_emb) -- stored to x. */
  int32_t pro, feats_dtype;
  const void* feats; void* x_in; const float* b_unify; const float* pe_rows;
  const int64_t* emb_ids; int64_t emb_ids_bs; const float* emb_table; const float* emb_pos;
} vct_layer_ss_desc;
typedef struct vct_ss_pack_seg { const void* w; int64_t ldw; int32_t nchunks; int32_t transposed; int64_t dst_chunk; } vct_ss_pack_seg;
int vct_layer_ss_supported(int dtype, int d, int H, int ff, int L, int Lm);
int64_t vct_layer_ss_stream_chunks(int ff, int cross);
int vct_ss_pack(const vct_ss_pack_seg* segs, int nseg, void* dst, void* stream);
int vct_layer_ss_fwd(const vct_layer_ss_desc* layers, int n_layers, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Sample-stationary BACKWARD of a self-attention + feed-forward layer stack (the activation-gradient chain; bf16, d = 512, 8 heads,
 * rows <= 32, <= 4 layers): ONE launch, one workgroup per sample, top layer first.
 * replaces: the autograd nodes of nn.TransformerEncoder's layers between the gradient of the stack output and the gradient of the
 * stack input (torch nn/modules/transformer.py:951-982 as built at MMEncoder.py:236-238): LayerNorm backward, linear2 / linear1 input
 * gradients with GELU' and dropout, out_proj input gradient, attention backward, in_proj input gradient.  The weight gradients are
 * NOT computed here: the kernel stores d f, d hpre, d a, d qkv (what vct_gemm_grouped multiplies with the saved activations) and one
 * partial (dgamma | dbeta) row per sample and LayerNorm ([B][2][512] fp32, the layout vct_ln_param_finalize_batched sums).
 * layers[0] is the TOP layer (last != 0: the stack-final norm is in front of it, y_last = that layer's output, dy = gradient of the
 * normed output); layers[n-1].dx receives the gradient of the stack input.  wpk: the transposed weight blocks in stream order,
 * vct_layer_ss_bwd_stream_chunks(ff) chunks per layer, layers back to back in processing order:
 *   [linear2.weight^T block j (vct_ss_pack transposed segment: w = W2 + 512 j, ld = ff) | linear1.weight^T K slice j (w = W1 + 512 j * 512,
 *    ld = 512)] for j < ff/512 | out_proj.weight^T (8 chunks) | in_proj_weight^T (24 chunks).
 * x / qkv / a / x1 / hpre / f, the statistics and the dropout sites are the forward's (vct_layer_ss_desc: x, qkv, a, n1, hpre, f, n3).
 * --------------------------------------------------------------------------------------------- */
typedef struct vct_ss_bwd_norm { const float* gamma; const float* mean; const float* rstd; float* ws; } vct_ss_bwd_norm;
typedef struct vct_layer_ss_bwd_desc {
  int32_t dtype, B, L, d, H, ff, act, last, causal, key_pad_shift;
  const void* wpk; int64_t nchunks;
  const void* dy; void* dx; const void* y_last;
  const void* x; const void* qkv; const void* a; const void* x1; const void* hpre; const void* f;
  vct_ss_bwd_norm n1, n3, nf;
  void* df; void* dhpre; void* da; void* dqkv;
  const uint8_t* key_pad; const int64_t* key_ids; int64_t key_ids_bs; int64_t pad_id;
  const uint32_t* seed; float p_drop;
  uint32_t site_sa, site_n1, site_ff, site_n3;
} vct_layer_ss_bwd_desc;
int64_t vct_layer_ss_bwd_stream_chunks(int ff);
int vct_layer_ss_bwd(const vct_layer_ss_bwd_desc* layers, int n_layers, void* stream);

/* ---------------------------------------------------------------------------------------------
 * y = LayerNorm(res + dropout(x)) (eps 1e-5, biased variance, affine); res may be NULL (plain LN).
 * replaces: dropoutN + residual add + nn.LayerNorm (torch nn/modules/transformer.py:951-957,
 * 1143-1153) and the stack-final norms (MMEncoder.py:238, CapDecoder.py:20).
 * mean/rstd: fp32 [M] saved for backward.
 * bwd: ds = dLN(dy) (gradient of the pre-norm sum), dxo = dropout-masked ds (may alias ds when p==0,
 * may be NULL when res == NULL and p == 0); dgamma/dbeta fp32 [d] (overwritten), param_ws fp32
 * [2 * vct_ln_ws_rows(M) * d] scratch.
 * --------------------------------------------------------------------------------------------- */
int vct_add_ln_fwd(int dtype, int M, int d, const void* x, const void* res, const float* gamma,
                   const float* beta, void* y, float* mean, float* rstd, const uint32_t* seed,
                   uint32_t site, float p_drop, void* stream);
/* the same with the stack-final norm behind it, one launch: y2 = LayerNorm2(y) (gamma2 / beta2), built on the rows of y as
 * stored -- the last layer's norm2 / norm3 + transformer_encoder.norm / decoder.norm (MMEncoder.py:238, CapDecoder.py:20) */
int vct_add_ln_ln_fwd(int dtype, int M, int d, const void* x, const void* res, const float* gamma, const float* beta,
                      void* y, float* mean, float* rstd, const float* gamma2, const float* beta2, void* y2, float* mean2,
                      float* rstd2, const uint32_t* seed, uint32_t site, float p_drop, void* stream);
int vct_add_ln_bwd(int dtype, int M, int d, const void* dy, const void* x, const void* res,
                   const float* gamma, const float* mean, const float* rstd, void* ds, void* dxo,
                   float* dgamma, float* dbeta, float* param_ws, const uint32_t* seed, uint32_t site,
                   float p_drop, void* stream);
/* the backward of vct_add_ln_ln_fwd in one launch: dy2 = gradient of y2 = LayerNorm2(y) (gamma2, mean2, rstd2; y as stored), then
 * vct_add_ln_bwd of y = LayerNorm(res + dropout(x)) on the gradient of y ROUNDED to the activation type -- bit-identical to the two
 * vct_add_ln_bwd launches it replaces (the gradient of y is not stored).  param_ws2 / param_ws: one partial-row set per norm
 * (dgamma / dbeta always deferred to vct_ln_param_finalize_batched).  replaces the autograd nodes of decoder.norm / encoder.norm
 * (CapDecoder.py:20, MMEncoder.py:238) and of the last layer's closing norm under `loss.backward()` (train.py:125). */
int vct_add_ln_ln_bwd(int dtype, int M, int d, const void* dy2, const void* y, const float* gamma2, const float* mean2,
                      const float* rstd2, float* param_ws2, const void* x, const void* res, const float* gamma,
                      const float* mean, const float* rstd, void* ds, void* dxo, float* param_ws, const uint32_t* seed,
                      uint32_t site, float p_drop, void* stream);
int vct_ln_ws_rows(int M);
/* dgamma == dbeta == NULL in vct_add_ln_bwd defers the column reduction of param_ws; this call then finalizes
 * n_entries LayerNorms in ONE launch.  table_dev: DEVICE int64 [n_entries][4] = {param_ws ptr, dgamma ptr,
 * dbeta ptr, vct_ln_ws_rows(M)} (every param_ws must stay untouched until then). */
int vct_ln_param_finalize_batched(const int64_t* table_dev, int n_entries, int d, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Encoder front end after the `unify` GEMM: z[b,0] = mean_t u[b,t] (all T rows, pads included),
 * z[b,t+1] = u[b,t] + pe_rows[t+1]  (pe_rows fp32 [T+1,d], row 0 = 0).
 * replaces: GlobalAggregation('avg') + cat + TemporalEncoding add (MMEncoder.py:196-197,248-250,
 * 89-104,271).  bwd: du[b,t] = dz[b,t+1] + dz[b,0]/T.
 * --------------------------------------------------------------------------------------------- */
int vct_enc_frontend_fwd(int dtype, int B, int T, int d, const void* u, const float* pe_rows, void* z,
                         void* stream);
int vct_enc_frontend_bwd(int dtype, int B, int T, int d, const void* dz, void* du, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Multi-modal encoder front end (n = 2 .. VCT_MM_MAX_MODAL feature streams) after the per-modality `unify` GEMMs
 * (csrc/vct_mm_frontend.hip).  Memory rows: modality i owns rows off_i .. off_i + T_i, off_i = sum_{j<i} (T_j + 1), S = off_n;
 * its row off_i is the aggregation row.
 *   fwd: x0[b, off_i]       = (temp[off_i] + modal_w[labels[off_i]]) + mean_t u_i[b, t]   (fp32 mean over all T_i rows, pads included)
 *        x0[b, off_i+1+t]   = (temp[off_i+1+t] + modal_w[labels[off_i+1+t]]) + u_i[b, t]
 *        key_pad[b, off_i] = 0, key_pad[b, off_i+1+t] = mask_i[b, t] (0 when mask_i is NULL); key_pad may be NULL.
 *   bwd: du_i[b, t] = dx[b, off_i+1+t] + dx[b, off_i] / T_i;  d_modal[l, :] = sum over b and the rows s with labels[s] == l of
 *        dx[b, s, :] -- WRITTEN (not accumulated), fp32, in a fixed order (no atomics: bitwise reproducible).
 * u_i / x0 / dx / du_i: dtype rows of d (16-byte aligned, d a multiple of 8 bf16 / 4 fp32); temp fp32 [S, d] (aggregation rows 0);
 * modal_w fp32 [n_labels, d]; labels int32 [S] in [0, n_labels) (not checked on the device: a row with a label outside it gets no
 * modal row and contributes to no d_modal row; the caller validates its table); n_labels = n or 2n; S <= 1024 here, but the
 * attention kernels that read x0 take S <= 64 (vct_attn_desc: Lq, Lk <= 64) and the sample-stationary stack S <= 32.
 * replaces: GlobalAggregation('avg') + cat + TemporalEncoding + ModalEmbedding + `temp + modal + feats` and the mask cat of
 * MultiModalEncoder.forward (MMEncoder.py:12-48,83-104,244-276), and their autograd backward.  One launch each.
 * --------------------------------------------------------------------------------------------- */
#define VCT_MM_MAX_MODAL 8
typedef struct vct_mm_frontend_desc {
  int32_t dtype, n, B, d;
  int32_t n_labels, reserved;
  int32_t T[VCT_MM_MAX_MODAL];
  const void* u[VCT_MM_MAX_MODAL];          /* fwd: [B*T_i, d] */
  const uint8_t* mask[VCT_MM_MAX_MODAL];    /* fwd: [B, T_i] (1 = padded) or NULL */
  const float* temp; const float* modal_w; const int32_t* labels;
  void* x0; uint8_t* key_pad;               /* fwd outputs: [B*S, d], [B, S] */
  const void* dx;                           /* bwd: [B*S, d] */
  void* du[VCT_MM_MAX_MODAL];               /* bwd: [B*T_i, d] */
  float* d_modal;                           /* bwd: [n_labels, d] */
} vct_mm_frontend_desc;
int vct_mm_frontend_fwd(const vct_mm_frontend_desc* d, void* stream);
int vct_mm_frontend_bwd(const vct_mm_frontend_desc* d, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Encoder front end with every option of the reference's `mme` block, n = 1 .. VCT_MM_MAX_MODAL feature streams
 * (csrc/vct_enc_frontend_ex.hip).  Row layout, vector width rules and the fixed-order reductions are those of vct_mm_frontend_*
 * (which, like vct_enc_frontend_*, stays the path of the shipped `avg` / `encoding` / no-norm combination).
 *   fwd, one launch:
 *        pre[b, off_i]     = (temporal(off_i)     + modal_w[labels[off_i]])     + agg_t u_i[b, t]
 *        pre[b, off_i+1+t] = (temporal(off_i+1+t) + modal_w[labels[off_i+1+t]]) + u_i[b, t]
 *        agg      = VCT_AGG_MEAN: fp32 mean, or VCT_AGG_MAX: maximum, over ALL T_i rows in row order, pads included
 *                   (GlobalAggregation 'avg' / 'max' = AdaptiveAvgPool1d(1) / AdaptiveMaxPool1d(1), MMEncoder.py:173-197)
 *        temporal = VCT_TEMPORAL_FIXED: temp[s] (fp32 [S, d], the TemporalEncoding rows, MMEncoder.py:83-104), or
 *                   VCT_TEMPORAL_LEARNED: emb_w[tidx[s]] (emb_w fp32 [emb_rows, d] = temp_emb.embedding.weight, tidx int32 [S] built by
 *                   the host: 0 on aggregation rows, linspace(1, T_0, T_i) as int32 on frame rows, MMEncoder.py:118-160; an index
 *                   outside [0, emb_rows) reads no row and gets no gradient)
 *        modal    = as vct_mm_frontend_fwd; n == 1 has none (modal_w, labels, d_modal unused and may be NULL, MMEncoder.py:232,271)
 *        x0 = pre, or with norm != 0:  x0 = dropout(LayerNorm(pre))  (gamma / beta fp32 [d], eps 1e-5; the dropout comes AFTER the
 *        norm, MMEncoder.py:240-242,272-273); mean / rstd fp32 [B*S] are stored for the backward; mask(site, b*S*d + s*d + c) of
 *        vct_common.h's counter hash, p_drop == 0 or seed == NULL: no dropout.  key_pad as vct_mm_frontend_fwd.
 *   bwd: dpre = dx, or with norm != 0 the LayerNorm backward of (dx x the same mask) per row, with pre recomputed from u in fp32;
 *        its column partials go to param_ws (fp32 [B*n][2][d]: one row pair per (sample, stream), to be finalized by
 *        vct_ln_param_finalize_batched with B*n rows) and dpre itself, in fp32, to the caller's buffer `dpre` [B*S, d].
 *        du_i[b, t] = dpre[b, off_i+1+t] + share of dpre[b, off_i]: / T_i (mean), or the whole value on the FIRST row that holds
 *        the column's maximum of u_i[b, :, c] (max; recomputed from u, which the caller keeps; ties go to the lower row like
 *        torch's max-pool backward).  d_modal as vct_mm_frontend_bwd.  d_emb fp32 [emb_rows, d] is WRITTEN in full: row e = sum over
 *        b and the rows s with tidx[s] == e of dpre[b, s, :], zeros where nobody reads e.  No atomics; bitwise reproducible.
 *        One launch; with norm != 0 and a modal or learned-temporal gradient to form, those sums over all samples run as a second
 *        launch behind the first (they read every sample's dpre; no in-launch hand-off between workgroups).
 * d a multiple of 8 (bf16) / 4 (fp32) and <= 1024 (a row lives in one wave's registers), S <= 1024, pointers 16-byte aligned.
 * --------------------------------------------------------------------------------------------- */
#define VCT_AGG_MEAN 0
#define VCT_AGG_MAX 1
#define VCT_TEMPORAL_FIXED 0
#define VCT_TEMPORAL_LEARNED 1
typedef struct vct_enc_frontend_ex_desc {
  int32_t dtype, n, B, d;
  int32_t n_labels, agg, temporal, norm;
  int32_t emb_rows; uint32_t site; float p_drop; int32_t reserved;
  int32_t T[VCT_MM_MAX_MODAL];
  const void* u[VCT_MM_MAX_MODAL];          /* fwd, and bwd when agg == MAX or norm: [B*T_i, d] */
  const uint8_t* mask[VCT_MM_MAX_MODAL];    /* fwd: [B, T_i] (1 = padded) or NULL */
  const float* temp;                        /* FIXED: [S, d] */
  const float* emb_w; const int32_t* tidx;  /* LEARNED: [emb_rows, d], [S] */
  const float* modal_w; const int32_t* labels;
  const float* gamma; const float* beta;    /* norm: [d] (beta: fwd only) */
  const uint32_t* seed;
  void* x0; uint8_t* key_pad;               /* fwd outputs: [B*S, d], [B, S] */
  float* mean; float* rstd;                 /* norm: [B*S], written by fwd, read by bwd */
  const void* dx;                           /* bwd: [B*S, d] */
  void* du[VCT_MM_MAX_MODAL];               /* bwd: [B*T_i, d] */
  float* d_modal;                           /* bwd, n >= 2: [n_labels, d] */
  float* d_emb;                             /* bwd, LEARNED: [emb_rows, d] */
  float* dpre; float* param_ws;             /* bwd, norm: fp32 [B*S, d], fp32 [B*n][2][d] */
} vct_enc_frontend_ex_desc;
int vct_enc_frontend_ex_fwd(const vct_enc_frontend_ex_desc* d, void* stream);
int vct_enc_frontend_ex_bwd(const vct_enc_frontend_ex_desc* d, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Row routing between the layers of the hierarchical multi-modal encoder (csrc/vct_hmm_mix.hip).  Stream j of the reference's
 * HMMEncoder passes through the LAST n_j of the L = max_j n_j shared layers: layer i takes, on the rows of stream j, the previous
 * layer's output when L - n_j < i and the stack input mm_src otherwise (MMEncoder.py:385-398).  The host turns that into one table
 * per layer, take uint8 [S]: 1 = the row continues from the previous layer's output, 0 = it restarts from the stack input.
 *   fwd:  x[b, s, :] = take[s] ? y[b, s, :] : x0[b, s, :]          bitwise copy, out of place, one launch
 *   bwd, from the gradient dx of a layer's input, one launch:
 *         dy[b, s, :]  = take[s] ? dx[b, s, :] : 0                  the gradient handed to the previous layer's output (exact zeros)
 *         acc[b, s, :]                                              fp32 [B*S, d], the stack input's gradient summed over the layers:
 *                        init != 0: WRITTEN, float(dx) on the restarting rows and 0 on the others (no memset precedes it);
 *                        init == 0: += float(dx) on the restarting rows, the others are not touched
 *         with dx0 != NULL (layer 0, where every row restarts): dx0 = round_to_dtype(acc + float(dx)); dy and acc are not written,
 *         take is not read (all may be NULL but acc); init must be 0.
 *   The sum runs per element in the order of the launches (top layer first); no atomics, bitwise reproducible run to run.
 * y / x0 / x / dx / dy / dx0: dtype rows of d (16-byte aligned, d a multiple of 8 bf16 / 4 fp32, VCT_E_ALIGN otherwise like the
 * front-end kernels); 1 <= S <= 1024.  Null pointers / bad enums: VCT_E_ARG, S or B out of range: VCT_E_SHAPE, before any device use.
 * --------------------------------------------------------------------------------------------- */
typedef struct vct_hmm_mix_desc {
  int32_t dtype, B, S, d;
  int32_t init, reserved;                   /* bwd: init != 0 writes acc instead of adding to it */
  const uint8_t* take;                      /* [S] */
  const void* y; const void* x0; void* x;   /* fwd: previous output, stack input -> layer input, each [B*S, d] */
  const void* dx;                           /* bwd: [B*S, d] */
  void* dy;                                 /* bwd: [B*S, d] (not with dx0) */
  float* acc;                               /* bwd: fp32 [B*S, d] */
  void* dx0;                                /* bwd, layer 0: [B*S, d] or NULL */
} vct_hmm_mix_desc;
int vct_hmm_mix_fwd(const vct_hmm_mix_desc* d, void* stream);
int vct_hmm_mix_bwd(const vct_hmm_mix_desc* d, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Token embedding: x[n] = dropout(table[ids[n]] + pos[n % S])   (no sqrt(d) scaling)
 * replaces: nn.Embedding(padding_idx) + PositionalEmbedding (CapDecoder.py:26,48; Embedding.py:23-25).
 * ids: int64 [N] read with element stride id_stride from ids + b*id_batch_stride (so the token-shift
 * view tgt[:, :-1] needs no copy): token n = (b = n / S, s = n % S) -> ids[b*id_batch_stride + s].
 * bwd: dtable fp32 [V,d] = scatter-add of dx rows (deterministic order), row pad_id zero.
 *      id_ws: int32 [id_ws_ints >= 2*V + 4 + B*S] scratch: first-occurrence / count tables (built with integer atomics) and the
 *      batch's ids in position order, which the NEXT call reads.  incremental != 0: dtable is known to be zero outside the rows of the ids of the PREVIOUS call (same
 *      dtable, same id_ws, nothing else writing dtable in between), so only those rows are zeroed (10 MB instead
 *      of 62.5 MB at cfg-B); incremental == 0 zeroes all V rows.
 * --------------------------------------------------------------------------------------------- */
int vct_embed_fwd(int dtype, int B, int S, int d, const int64_t* ids, int64_t id_batch_stride,
                  const void* table, const float* pos, void* x, const uint32_t* seed, uint32_t site,
                  float p_drop, void* stream);
/* ---------------------------------------------------------------------------------------------
 * The frozen CLIP text tower (text.py): the two kernels that the rest of the library cannot express.  Forward only.
 * vct_preln_fwd: y[M, d] = LayerNorm(x[M, d]) (eps 1e-5, biased variance, affine).  x is the FP32 residual stream of a pre-LN stack,
 *   y has out_dtype (VCT_F32 | VCT_BF16); no statistics are saved.  replaces: `ln_1` / `ln_2` of CLIP's ResidualAttentionBlock
 *   (clip/model.py, as reached from the reference's model/TextEncoder.py).
 * vct_text_pool: per caption b, e_b = the FIRST index of the maximum of ids[b, 0 .. Lids) (CLIP: `text.argmax(dim=-1)`, the EOT token
 *   has the largest id); y[b] = LayerNorm(x[b * L + e_b]) in out_dtype (gamma / beta = ln_final); eot[b] = e_b (int32).
 *   ids: int64 [B, ld_ids]; x: fp32 [B * L, d], the stream of the first L <= Lids positions.  e_b >= L (the caller trimmed behind the
 *   EOT) sets *err = 1 (device int32, never cleared here) and writes a zero row -- the caller reads err when it chooses to.
 *   replaces: `x[arange(B), text.argmax(-1)]` between ln_final and text_projection (clip/model.py, encode_text).
 * d a multiple of 4 (VCT_E_ALIGN) up to 1024 (VCT_E_SHAPE); M, B, L >= 1, Lids >= L, ld_ids >= Lids (VCT_E_SHAPE); x / gamma / beta and
 * an fp32 y 16-byte, a bf16 y and ids 8-byte, eot / err 4-byte aligned (VCT_E_ALIGN); NULL operand / bad dtype: VCT_E_ARG.  All
 * before any device use.
 * --------------------------------------------------------------------------------------------- */
int vct_preln_fwd(int out_dtype, int M, int d, const float* x, const float* gamma, const float* beta, void* y, void* stream);
int vct_text_pool(int out_dtype, int B, int L, int Lids, int d, const int64_t* ids, int64_t ld_ids, const float* x,
                  const float* gamma, const float* beta, void* y, int32_t* eot, int32_t* err, void* stream);
/* ---------------------------------------------------------------------------------------------
 * The frozen CLIP vision tower (vision.py): the three kernels around the pre-LN block, which is vct_preln_fwd, vct_gemm
 * and vct_attn_fwd as in the text tower.  Forward only.
 * vct_frames_to_patches: uint8 RGB frames [N, H, W, 3] -> the patch-embedding GEMM's A operand,
 *     out[(n * G + gy) * G + gx, c * P * P + py * P + px],  G = R / P,  in out_dtype (VCT_F32 | VCT_BF16): the row layout of
 *   conv1.weight.view(width, 3 * P * P).  The image is PIL's integer bicubic resize (shorter side to R, the longer to
 *   int(R * long / short)), centre-cropped to R x R: horizontal pass first, the vertical pass on its uint8 result, int32 accumulators
 *   that start at 2^21, are shifted right by 22 and clamped to 0 .. 255.  The HOST decides every window and weight: hx_min / hx_len
 *   [R] and hx_w [R, kx] (int32, 22-bit fixed point, zero-padded) describe the R cropped columns of the horizontal pass in input
 *   columns, vy_* [R] / [R, ky] the R cropped rows of the vertical pass in input rows; a pass PIL skips (the size does not change) is
 *   the one-tap table of weight 2^22.  lut: [3][256] in out_dtype, the value of every byte per channel (ToTensor + Normalize as the
 *   host computed it); the kernel only looks it up, so every output element is one of the table's.  stage_rows: the largest number of
 *   input rows the P rows of one patch read (max over gy of vy_min[gy P + P - 1] + vy_len[gy P + P - 1] - vy_min[gy P]); the
 *   horizontal pass of those rows is staged in LDS as uint8.  crop (NULL: not written): the cropped image, uint8 [N, R, R, 3].
 *   One launch for any N, one workgroup per (frame, patch); windows are clamped to the frame and to stage_rows on the device.
 *   replaces: clip's `_transform` (Resize(BICUBIC), CenterCrop, ToTensor, Normalize on a PIL image) and the unfold of `conv1` in
 *   VisionTransformer.forward (clip/model.py), as reached from the reference's predict_video.py --video.
 *   NULL operand / bad dtype: VCT_E_ARG; N, H, W, R, P, kx, ky, stage_rows < 1, R % P, kx > W, ky or stage_rows > H, N * G * G or
 *   3 * H * W beyond int32, or tables + staging + one patch (4 P (kx + ky + 4) + 3 P stage_rows + 3 P P bytes) over 64 KB of LDS:
 *   VCT_E_SHAPE; P not a multiple of 8, out not 16-byte, a table, an fp32 lut or crop not 4-byte aligned: VCT_E_ALIGN.
 * vct_vit_embed: s[n, 0] = cls + pos[0], s[n, 1 + g] = e[n * (L - 1) + g] + pos[1 + g]; x[n * L + l] = LayerNorm(s[n, l]) (gamma /
 *   beta = ln_pre, eps 1e-5).  e: fp32 [N * (L - 1), d], the patch GEMM's output; x: the fp32 residual stream [N * L, d].
 *   replaces: the class-token concatenation, `+ positional_embedding` and `ln_pre` of VisionTransformer.forward.
 * vct_vit_pool: y[n] = LayerNorm(x[n * L]) in out_dtype (gamma / beta = ln_post): the class rows only; no other row is read.
 *   replaces: `ln_post(x[:, 0, :])` in front of `@ proj`.
 * Both: d a multiple of 4 (VCT_E_ALIGN) up to 1024 (VCT_E_SHAPE); N >= 1, L >= 2 (embed) / 1 (pool) (VCT_E_SHAPE); every fp32 operand
 * 16-byte, a bf16 y 8-byte aligned (VCT_E_ALIGN); NULL operand / bad dtype: VCT_E_ARG.  All before any device use.
 * --------------------------------------------------------------------------------------------- */
int vct_frames_to_patches(int out_dtype, int N, int H, int W, int R, int P, const uint8_t* frames, const int32_t* hx_min,
                          const int32_t* hx_len, const int32_t* hx_w, int kx, const int32_t* vy_min, const int32_t* vy_len,
                          const int32_t* vy_w, int ky, int stage_rows, const void* lut, void* out, uint8_t* crop, void* stream);
int vct_vit_embed(int N, int L, int d, const float* e, const float* cls, const float* pos, const float* gamma, const float* beta,
                  float* x, void* stream);
int vct_vit_pool(int out_dtype, int N, int L, int d, const float* x, const float* gamma, const float* beta, void* y, void* stream);

int vct_embed_bwd(int dtype, int B, int S, int d, int V, const int64_t* ids, int64_t id_batch_stride,
                  int64_t pad_id, const void* dx, float* dtable, int32_t* id_ws, int64_t id_ws_ints, int incremental,
                  const uint32_t* seed, uint32_t site, float p_drop, void* stream);
/* vct_embed_bwd that ALSO marks the rows it writes in a per-row "live" table (uint8 [V], device; NULL: no table): live[id] = 1 for
 * every id of the batch that is inside [0, V) and is not pad_id -- exactly the rows that receive a gradient.  The table is never
 * cleared by a call: it accumulates "every token id any batch has used so far", which is what the optimizer's row-aware pass
 * (vct_adam_step_ranges_rows) steps.  An id outside [0, V) owns no row, with or without a table.  No reference counterpart. */
int vct_embed_bwd_live(int dtype, int B, int S, int d, int V, const int64_t* ids, int64_t id_batch_stride,
                       int64_t pad_id, const void* dx, float* dtable, int32_t* id_ws, int64_t id_ws_ints, int incremental,
                       const uint32_t* seed, uint32_t site, float p_drop, uint8_t* live, void* stream);
/* live[r] = 1 when any element of row r of exp_avg_rows, exp_avg_sq_rows or (when not NULL) grad_rows has a bit set, else 0
 * ([V, d] fp32, contiguous): the table rebuilt from the buffers -- when it is created, after an optimizer state was loaded, after
 * anything but the row-aware pass stepped the table. */
int vct_embed_live_rebuild(int32_t V, int32_t d, const float* grad_rows, const float* exp_avg_rows, const float* exp_avg_sq_rows,
                           uint8_t* live, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The caption losses over the vocabulary logits (csrc/vct_caption_loss.hip): vct_sce_loss, vct_sce_loss_ls, vct_wce_loss -- one
 * kernel family.  Each returns the loss and, unless dlogits is NULL, its gradient w.r.t. the logits; one workgroup per row, the row
 * held in registers (one HBM read + one exp + one HBM write per logit).  What the three share:
 *   logits [N, ldl] (V valid columns); labels int64: row n = (b = n / S, s = n % S) ->
 *   labels[b*label_batch_stride + s]  (so tgt[:, 1:] needs no copy); row n is valid when its label y != pad_id;
 *   count = number of valid rows;  lse, p over the V columns.
 *   loss_out fp32 [1]; dlogits (may alias logits; columns V..ld_dl-1 are written as 0) or NULL = forward only; ld_dl is ignored
 *   when dlogits is NULL.
 *   Limits: ldl, ld_dl multiples of 8 (bf16) / 4 (fp32), >= V rounded up to that, and <= 65536 (bf16) / 32768 (fp32) columns;
 *   logits and dlogits 16-byte aligned.  VCT_E_ARG: bad dtype / NULL logits, labels, loss_out or row_ws; VCT_E_SHAPE: N, S, V <= 0,
 *   N not a multiple of S, a row wider than the limit; VCT_E_ALIGN: ldl / ld_dl / a base address off the rules above.
 *   A label outside [0, V) on a valid row is computed against column 0 (no stray access) and turns the loss into NaN.
 *   count == 0: the loss is 0 / 0 = NaN, every gradient row is zero.
 *   Two calls are bitwise equal (fixed-order single-workgroup count and finalise, no float atomics).
 *
 * vct_sce_loss: symmetric cross-entropy,  loss = alpha * sum CE_n / count + (1 - alpha) * mean over all N rows of RCE_n.
 * replaces: SCELoss.forward (loss.py:78-92) / nn.CrossEntropyLoss(ignore_index) when alpha == 1
 * (CapDecoder.py:28-32,56-59) and their autograd backward.
 *   row_ws fp32 [2*N + 2] scratch.
 * --------------------------------------------------------------------------------------------- */
int vct_sce_loss(int dtype, int N, int S, int V, const void* logits, int64_t ldl, const int64_t* labels,
                 int64_t label_batch_stride, int64_t pad_id, float alpha, float* loss_out, void* dlogits,
                 int64_t ld_dl, float* row_ws, void* stream);

/* ---------------------------------------------------------------------------------------------
 * vct_sce_loss with label smoothing on its CE term, plus the un-smoothed NLL and the token accuracy.
 * replaces: nn.CrossEntropyLoss(ignore_index, label_smoothing) at alpha == 1; the reference's SCELoss has no smoothing -- with
 * alpha < 1 the CE term is smoothed and the RCE term is vct_sce_loss's, unchanged.
 *   eps = smoothing in [0, 1)
 *   nll_n = lse - x[y];  smooth_n = lse - (1/V) sum_{j<V} x[j];  ce_n = (1 - eps) nll_n + eps smooth_n  (0 on pad rows)
 *   loss_out[0] = alpha * sum ce_n / count + (1 - alpha) * L_rce               (L_rce: vct_sce_loss's, mean over all N rows)
 *   dlogits[n, j] = (alpha / count) (p_j - (1 - eps) [j == y] - eps / V) [valid] + vct_sce_loss's RCE part; columns V..ld_dl-1 = 0
 *   stats_out[0] = sum over valid n of nll_n / count;  stats_out[1] = #{valid n: x[y] == max_j x[j]} / count (a tie with the
 *   maximum counts as a hit; a label outside the vocabulary as a miss)                              (fp32 [2] or NULL)
 * smoothing == 0 gives vct_sce_loss's loss_out and dlogits bit for bit.  smoothing outside [0, 1) or NaN: VCT_E_ARG, nothing
 * launched.  The out-of-vocabulary label also makes stats_out[0] NaN.  row_ws fp32 [4*N + 2] scratch.
 * --------------------------------------------------------------------------------------------- */
int vct_sce_loss_ls(int dtype, int N, int S, int V, const void* logits, int64_t ldl, const int64_t* labels,
                    int64_t label_batch_stride, int64_t pad_id, float alpha, float smoothing, float* loss_out,
                    float* stats_out, void* dlogits, int64_t ld_dl, float* row_ws, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Sequence-weighted cross-entropy for self-critical sequence training: vct_sce_loss at alpha = 1 with
 * one weight (the advantage) per sequence.  The reference has no policy-gradient stage; the semantics are DESIGN.md's.
 *   row n belongs to sequence b = n / S;  logp_n = x[y] - max - log(sum exp(x - max)) in fp32
 *   loss_out[0] = -(sum over valid n of seq_w[b] * logp_n) / count
 *   tok_logp[n] = logp_n on valid rows, exactly 0 on pad rows                                  (fp32 [N] or NULL)
 *   dlogits[n, j] = (seq_w[b] / count) * (p_j - [j == y]) on valid rows, exact zeros on pad rows and in columns V..ld_dl-1.
 * seq_w: DEVICE fp32 [N / S], read by the kernel (a recording stays valid across steps), or NULL = all ones.  With NULL or with
 * all 1.0f, loss and dlogits are bitwise those of vct_sce_loss(alpha = 1).  row_ws fp32 [2*N + 2] scratch.
 * --------------------------------------------------------------------------------------------- */
int vct_wce_loss(int dtype, int N, int S, int V, const void* logits, int64_t ldl, const int64_t* labels,
                 int64_t label_batch_stride, int64_t pad_id, const float* seq_w, float* loss_out, float* tok_logp,
                 void* dlogits, int64_t ld_dl, float* row_ws, void* stream);

/* (csrc/vct_caption_loss.hip)  out[g*R + r, :] = sum over n < G of in[(g*G + n)*R + r, :] for g < B, r < R: `in` [B*G*R, d] and `out` [B*R, d] contiguous rows
 * of the compute dtype, 16-byte aligned, d a multiple of 8 (bf16) / 4 (fp32).  fp32 accumulation in ascending n, one rounding into
 * the compute dtype; G = 1 is a bitwise copy.  Folds d(memory) of G sampled captions per video back onto the video's memory rows.
 * VCT_E_ARG: bad dtype / NULL; VCT_E_SHAPE: B, G, R, d <= 0 or d not a multiple of the vector; VCT_E_ALIGN: misaligned base. */
int vct_group_sum(int dtype, int B, int G, int R, int d, const void* in, void* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The self-critical reward on the device (csrc/vct_cider.hip): CIDEr-D of sampled token ids against device-resident reference
 * tables, and the advantages in the layout of vct_wce_loss's seq_w.  The reference has no policy-gradient stage; the semantics
 * are rewards.CiderD / rewards.advantages, and the tables are built on the host by rewards.CiderD.device_tables().
 *
 * Keys.  An n-gram of order k <= VCT_CIDER_MAX_ORDER is four int32 words: its k token ids (>= 0), then -1 padding, so the order
 * is part of the key.  Keys are compared exactly, word by word; ordered lexicographically as signed words.
 * Hash of a key (uint32 arithmetic; the numpy builder and the kernel both implement THIS):
 *     h = 0x811C9DC5;  for each of the four words w, in order:  h = (h ^ (uint32)w) * 0x01000193;
 *     h ^= h >> 16;  h *= 0x85EBCA6B;  h ^= h >> 13;  h *= 0xC2B2AE35;  h ^= h >> 16;        slot = h & (table_cap - 1)
 * Corpus table: open addressing, linear probing (slot, slot + 1, ... modulo table_cap), table_cap a power of two >= twice the
 * number of unique corpus n-grams.  Slot s: table_keys[4 * s .. 4 * s + 3] and table_idf[s] = log(#videos) - log(max(1, df)) in
 * fp64 (the host's own value; the kernel takes no logarithm); an empty slot has key word 0 == -1.  A lookup ends at the key
 * (found), at an empty slot or after table_cap probes (absent: idf = log_nvid); a collision costs probes, never a score.
 * Per video v < n_videos (CSR): its references are vid_ref_ptr[v] .. vid_ref_ptr[v + 1] - 1; per reference r: ref_len[r] (tokens
 * after the cut), ref_norm[4 * r + k] (the norm of order k + 1; 0 beyond n) and its unique n-grams ent_keys / ent_w at
 * ref_ent_ptr[r] .. ref_ent_ptr[r + 1] - 1, SORTED by key (the kernel searches them by bisection), ent_w = tf * idf in fp64.
 *
 * vct_cider_d: one 256-thread workgroup per candidate (b, s), b < B, s < N.  The candidate is ids[b, s, 1 .. L] through the
 * element strides (column 0 is the start token and is not read), cut after its first end_id (kept); a row without one is taken
 * whole; nothing behind the end token reaches the score.  A token id outside [0, 2^31) matches no table entry.  Orders 1 .. n:
 *     c_w = tf(w) * idf(w);  |c|_k = sqrt(sum_w c_w^2);  sim_k(c, r) = sum_w min(c_w, r_w) * r_w / (|c|_k |r|_k)  (skipped when
 *     either norm is 0), times exp(-(len c - len r)^2 / two_sigma_sq);  reward[b * N + s] = (float)(10 * sum / (n * R)),
 * R = the video's reference count; R == 0 (or vid_rows[b] outside [0, n_videos)) scores exactly 0.  Everything behind the
 * integer counts is fp64, every sum runs serially in first-occurrence order of the candidate's n-grams (the host's order), no
 * floating-point atomics: two calls agree bitwise.
 * VCT_E_ARG: NULL descriptor / operand; VCT_E_SHAPE: B, N < 1, L < 0 or L > VCT_CIDER_MAX_LEN, n outside 1 .. VCT_CIDER_MAX_ORDER,
 * table_cap not a power of two, B * N > 2^31 - 1; VCT_E_ALIGN: an fp64 table not 8-byte or a key table not 16-byte aligned.
 *
 * vct_scst_advantages: rewards fp32 [B, N] -> adv fp32 [B * N] (may alias rewards), base_out fp32 [B], means fp32 [2] =
 * {mean reward, mean baseline}.  baseline == NULL (needs N >= 2, else VCT_E_SHAPE): the leave-one-out mean
 * base = (sum_n r - r) / (N - 1) in fp64, adv = (float)(r - base), base_out[b] = (float)(sum_n r / N) (the mean of the video's N
 * leave-one-out baselines).  baseline fp32 [B]: adv = (float)((double)r - baseline[b]), base_out[b] = baseline[b].  The means
 * are fp64 sums over b (of sum_n r, of the baseline) by ONE workgroup in a fixed order, divided by B * N and B, rounded once.
 * --------------------------------------------------------------------------------------------- */
#define VCT_CIDER_MAX_LEN 64
#define VCT_CIDER_MAX_ORDER 4
typedef struct vct_cider_desc {
  int32_t B, N, L, n;            /* L: candidate tokens after the start column */
  const int64_t* ids;            /* [B, N, 1 + L] through the strides below (elements); points at column 0 */
  int64_t stride_b, stride_n, stride_l;
  int64_t end_id;
  double log_nvid, two_sigma_sq;
  const int32_t* vid_rows;       /* [B]: the table row of each video */
  int32_t n_videos, table_cap;
  const int32_t* table_keys;     /* [table_cap, 4] */
  const double* table_idf;       /* [table_cap] */
  const int32_t* vid_ref_ptr;    /* [n_videos + 1] */
  const int32_t* ref_len;        /* [R_total] */
  const double* ref_norm;        /* [R_total, 4] */
  const int32_t* ref_ent_ptr;    /* [R_total + 1] */
  const int32_t* ent_keys;       /* [E_total, 4] */
  const double* ent_w;           /* [E_total] */
  float* reward;                 /* [B * N] */
} vct_cider_desc;
int vct_cider_d(const vct_cider_desc* d, void* stream);
int vct_scst_advantages(int B, int N, const float* rewards, const float* baseline, float* adv, float* base_out, float* means,
                        void* stream);

/* ---------------------------------------------------------------------------------------------
 * Caption metrics for evaluation on the device (csrc/vct_capmetric.hip, csrc/vct_cider.hip): BLEU-1..4 ("closest" reference
 * length, corpus level), ROUGE-L (beta = 1.2) and CIDEr of decoded token ids, as coco-caption's Bleu(4), Rouge() and Cider()
 * compute them on tokenised strings (eval.py:42-123 scores through them).  METEOR is absent (Java + WordNet data).  The semantics
 * are metrics.CaptionMetrics; the tables are built on the host by metrics.CaptionMetrics.device_tables().
 *
 * Conventions of all three entry points.  A candidate is ids[c, 1 .. L] through the element strides (column 0 is the start token
 * and is not read), cut BEFORE its first end_id: the end token is dropped and nothing behind it reaches any output; a row without
 * one is taken whole; L <= VCT_CIDER_MAX_LEN.  A candidate id outside [0, 2^31) matches nothing.  References carry no start or end
 * token and may have any length; they are CSR over the video's table row v = vid_rows[c]: references vid_ref_ptr[v] ..
 * vid_ref_ptr[v + 1] - 1 (the SAME array as vct_cider_desc's), tokens of reference r: ref_tok[ref_tok_ptr[r] .. ref_tok_ptr[r + 1] - 1],
 * each in [0, 2^31).  A video without references (or a row outside [0, n_videos)) gives an all-zero row everywhere.
 *
 * vct_capmetric_counts: one 256-thread workgroup per caption c < C.  counts[12 * c ..] = {len, reflen, correct_1..4, guess_1..4,
 * lcs_max, 0}:  len = tokens after the cut;  reflen = the reference length minimising (|len_r - len|, len_r) (a tie goes to the
 * shorter reference; an empty candidate gets the shortest);  guess_k = max(0, len - k + 1);  correct_k = sum over the candidate's
 * distinct k-grams w of min(count_c(w), max_r count_r(w));  lcs_max = max_r LCS(candidate, reference r).
 * rouge[3 * c ..] = {prec, rec, F}:  prec = lcs_max / len,  rec = max_r LCS_r / len_r (an empty reference contributes 0),
 * F = (1 + beta_sq) * prec * rec / (rec + beta_sq * prec) when both are non-zero, else 0; each of prec and rec is ONE fp64 division
 * of two integers (rec's maximum is found by integer cross-multiplication).  The n-gram counts compare token arrays directly
 * (wave k holds order k + 1, lane p the instance that starts at token p); the LCS is the bit-parallel row recurrence on one
 * 64-bit word per wave (lane j holds candidate token j; per reference token, M = ballot(match), U = V & M, V = (V + U) | (V - U)
 * from all ones; LCS = zero bits among the low len bits of V), the group's waves striding over the references.  All integer
 * outputs are exact, there is no floating-point atomic and no data-dependent order: two calls agree bitwise.
 * VCT_E_ARG: NULL descriptor / operand or beta_sq not > 0; VCT_E_SHAPE: C < 1, L < 0 or L > VCT_CIDER_MAX_LEN, n_videos < 0;
 * VCT_E_ALIGN: ids or rouge not 8-byte, an int32 array not 4-byte aligned.
 *
 * vct_cider_d_eval: vct_cider_d's kernel (same descriptor, same tables, same order of every sum) with the cut BEFORE the end token;
 * writes the un-rounded fp64 score[b * N + s] = 10 * sum / (n * R), and also (float) of it to d->reward when that is not NULL.
 * Refusals as vct_cider_d (reward may be NULL; score NULL: VCT_E_ARG, not 8-byte aligned: VCT_E_ALIGN).
 *
 * vct_capmetric_finish: ONE 256-thread workgroup folds the C rows: int64 sums of {len, reflen, correct_k, guess_k}, fp64 sums of
 * F and (cider != NULL) of cider[c], thread t taking rows t, t + 256, ..., then a fixed-order tree.  With tiny = 1e-15, small = 1e-9:
 *     p = 1;  for k = 1..4:  p *= (correct_k + tiny) / (guess_k + small),  Bleu_k = pow(p, 1 / k);
 *     ratio = (len + tiny) / (reflen + small);  if ratio < 1 every Bleu_k *= exp(1 - 1 / ratio)
 * out[8] = {Bleu_1, Bleu_2, Bleu_3, Bleu_4, ROUGE_L = mean F, CIDEr = mean cider (0 without), Bleu_4 + ROUGE_L + CIDEr, (double)C}.
 * VCT_E_ARG: NULL counts / rouge / out; VCT_E_SHAPE: C < 1; VCT_E_ALIGN: an fp64 buffer not 8-byte, counts not 4-byte aligned.
 * --------------------------------------------------------------------------------------------- */
#define VCT_CAPMETRIC_COUNT_COLS 12
typedef struct vct_capmetric_desc {
  int32_t C, L;                  /* captions; candidate tokens after the start column */
  const int64_t* ids;            /* [C, 1 + L] through the strides below (elements); points at column 0 */
  int64_t stride_c, stride_l;
  int64_t end_id;
  const int32_t* vid_rows;       /* [C]: the table row of each caption's video */
  int32_t n_videos, reserved;
  double beta_sq;
  const int32_t* vid_ref_ptr;    /* [n_videos + 1] */
  const int32_t* ref_tok_ptr;    /* [R_total + 1] */
  const int32_t* ref_tok;        /* [T_total] */
  int32_t* counts;               /* [C, 12] */
  double* rouge;                 /* [C, 3] */
} vct_capmetric_desc;
int vct_capmetric_counts(const vct_capmetric_desc* d, void* stream);
int vct_cider_d_eval(const vct_cider_desc* d, double* score, void* stream);
int vct_capmetric_finish(int C, const int32_t* counts, const double* rouge, const double* cider, double* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The video-text matching head (csrc/vct_match.hip), fp32 end to end.
 * replaces: ClipSymmetricalLoss / ClipSymmetricalLoss_WithDualSoftmax (loss.py:7-67) as called by Matching.forward
 * (Matching.py:27-30: loss_fn(text_feat, vid_feat)) and their autograd backward.
 *   sim[i, j] = t^_i . v^_j, both sides L2-normalised per row (text rows i, video columns j; no epsilon, as the reference)
 *   CSL:      logits = sim * exp(*temp) (VCT_MATCH_TEMP_EXP) or sim (VCT_MATCH_TEMP_NONE)
 *   CSL_WDS:  logits = sim * softmax(sim / *temp, over i) * B     (VCT_MATCH_TEMP_DIV only)
 *   loss = (CE(logits, arange) + CE(logits^T, arange)) / 2, mean reduction.
 * text / vid [B, Dt] with leading dimensions (multiples of 4, 16-byte aligned bases); temp: DEVICE scalar, NULL exactly when
 * temp_kind is VCT_MATCH_TEMP_NONE.  loss [1].  dvid [B, Dt] or NULL (= forward only): the gradient w.r.t. the UN-normalised vid.
 * dtemp [1] or NULL: written only when temp and dvid are given.  sim [B, ld_sim] or NULL: the logits as the loss saw them.
 * 1 <= B <= 256, Dt a multiple of 4 up to 1024 (VCT_E_SHAPE otherwise); workspace: vct_match_loss_workspace_bytes(B, Dt) bytes
 * (0 for an unsupported shape), 16-byte aligned, owned by the caller.  No allocation, no synchronisation, no host read; every
 * reduction has a fixed order and there is no floating-point atomic: two calls on the same inputs agree bitwise, and a
 * forward-only call returns the same loss bits.  Launches: CSL 4 (3 forward only), CSL_WDS 5 (4 forward only).
 * --------------------------------------------------------------------------------------------- */
enum { VCT_MATCH_CSL = 0, VCT_MATCH_CSL_WDS = 1 };
enum { VCT_MATCH_TEMP_NONE = 0, VCT_MATCH_TEMP_EXP = 1, VCT_MATCH_TEMP_DIV = 2 };
typedef struct vct_match_loss_desc {
  int32_t B, Dt, loss_kind, temp_kind;
  const float* text; int64_t ld_text;
  const float* vid; int64_t ld_vid;
  const float* temp;
  float* loss;
  float* dvid; int64_t ld_dvid;
  float* dtemp;
  float* sim; int64_t ld_sim;
  void* workspace; int64_t workspace_bytes;
} vct_match_loss_desc;
int vct_match_loss(const vct_match_loss_desc* d, void* stream);
int64_t vct_match_loss_workspace_bytes(int B, int Dt);

/* The aggregation row of every sample <-> the matching head (MMEncoder.py: agg_feat = memory[:, 0]), and the mix of the two tasks'
 * gradients of `memory` (MMT4Caption.py:146: loss_beta * cap_loss + (1 - loss_beta) * match_loss).
 *   fwd: agg[b, :] = float(mem[b * Te, :])                                                     mem [B * Te, d] of dtype, agg fp32 [B, d]
 *   bwd: dmem[b * Te + r, :] = beta * dmem[b * Te + r, :] + (r == 0 ? (1 - beta) * dagg[b, :] : 0)   over the whole [B * Te, d], in place
 *        (fp32 products rounded separately, one add, one rounding to dtype); empty != 0: dmem holds nothing yet and is NOT read
 *        (the match task: beta = 0, no zero fill needed).
 * d a multiple of 8 (bf16) / 4 (fp32), 16-byte aligned bases (VCT_E_ALIGN); 0 <= beta <= 1 (VCT_E_ARG). */
typedef struct vct_match_agg_desc {
  int32_t dtype, B, Te, d;
  int32_t empty; float beta;
  const void* mem; float* agg;       /* fwd */
  const float* dagg; void* dmem;     /* bwd */
} vct_match_agg_desc;
int vct_match_agg_fwd(const vct_match_agg_desc* d, void* stream);
int vct_match_agg_bwd(const vct_match_agg_desc* d, void* stream);

/* x[0 .. n) *= s (fp32, 16-byte aligned base): the caption task's share of the flat gradient buffer times loss_beta. */
int vct_scale(float* x, int64_t n, float s, void* stream);
/* out[0 .. n) = a * x + b * y (fp32; y NULL: a * x; out may alias x or y): loss = loss_beta * cap_loss + (1 - loss_beta) * match_loss
 * on the device, and small scaled copies between the head's buffers and the flat gradient buffer. */
int vct_axpby(float* out, const float* x, float a, const float* y, float b, int64_t n, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Text-video retrieval evaluation of the matching head (csrc/vct_retrieval.hip), fp32 end to end: the ranks of text->video and
 * video->text retrieval over a whole split and their statistics, without ever storing the [Nt, Nv] score matrix.
 *   text [Nt, Dt], vid [Nv, Dt] with leading dimensions; gt int32 [Nt]: the video row each text belongs to (any number of texts per
 *   video, in any order, possibly none).  s[i, j] = t^_i . v^_j as in vct_match_loss (rows L2-normalised, no epsilon).
 *   VCT_RETRIEVAL_PLAIN:         f = s (CSL's exp(temp) factor is monotone and dropped)
 *   VCT_RETRIEVAL_DUAL_SOFTMAX:  f[i, j] = s[i, j] * softmax_i(s[:, j] / *tau)[i] (what CSL_WDS trains, without its factor B);
 *                                tau: DEVICE scalar, non-NULL exactly in this mode.
 * Ranks are 1-based, ties go to the lower index (a stable descending sort):
 *   ranks_t2v[i] = 1 + #{ j : f[i,j] > f[i,g] or (f[i,j] == f[i,g] and j < g) },  g = gt[i]
 *   ranks_v2t[j] = 1 + #{ i : f[i,j] > f[i*,j] or (f[i,j] == f[i*,j] and i < i*) },  i* the best-scoring own text of video j (the
 *                  lowest index on ties): the best-ranked-own-caption convention of multi-sentence retrieval.
 * A video without a text, and a text whose gt is outside [0, Nv) (never used as an index), get rank 0 and enter no statistic; such
 * a text still competes in video->text and takes part in the column softmax.
 * out[12]: per direction (text->video, then video->text) {R@1, R@5, R@10 as fractions, median rank (numpy's: the mean of the two
 * middle ranks of an even count), mean rank, number of queries counted}; all zero for a direction without a query.
 * f[i, j] has the same bits wherever it is computed (one fixed summation order over Dt, the inverse norms computed once), so the
 * comparisons above compare like with like at any tile position and for any Nt / Nv.  Integer atomics only; the column
 * statistics of the dual softmax are per-tile partials folded in tile order: two calls on the same inputs agree bitwise.
 * Plain: one sweep over the matrix; dual softmax: one more before it for the column statistics.  phases: 0 = everything; else a
 * bit set of VCT_RETRIEVAL_PH_* to run (timing one phase; a phase reads what the earlier ones left in the workspace and outputs).
 * Dt a multiple of 4 up to 1024, 1 <= Nt, Nv <= 2^20, ld >= Dt (VCT_E_SHAPE); ld a multiple of 4, text / vid / workspace 16-byte,
 * out 8-byte, the int32 arrays 4-byte aligned (VCT_E_ALIGN); NULL operand, bad mode / phases, tau missing or unexpected (VCT_E_ARG);
 * workspace: vct_retrieval_workspace_bytes(Nt, Nv, Dt, mode) bytes (0 for an unsupported shape or mode), owned by the caller
 * (VCT_E_WORKSPACE).  No allocation, no synchronisation, no host read.
 * --------------------------------------------------------------------------------------------- */
enum { VCT_RETRIEVAL_PLAIN = 0, VCT_RETRIEVAL_DUAL_SOFTMAX = 1 };
enum { VCT_RETRIEVAL_PH_PREP = 1, VCT_RETRIEVAL_PH_STATS = 2, VCT_RETRIEVAL_PH_GT = 4, VCT_RETRIEVAL_PH_COUNT = 8,
       VCT_RETRIEVAL_PH_FINISH = 16 };
typedef struct vct_retrieval_desc {
  int32_t Nt, Nv, Dt, mode;
  const float* text; int64_t ld_text;
  const float* vid; int64_t ld_vid;
  const int32_t* gt;             /* [Nt] */
  const float* tau;
  int32_t* ranks_t2v;            /* [Nt] */
  int32_t* ranks_v2t;            /* [Nv] */
  double* out;                   /* [12] */
  void* workspace; int64_t workspace_bytes;
  int32_t phases, reserved;
} vct_retrieval_desc;
int vct_retrieval_ranks(const vct_retrieval_desc* d, void* stream);
int64_t vct_retrieval_workspace_bytes(int Nt, int Nv, int Dt, int mode);

/* ---------------------------------------------------------------------------------------------
 * Batch assembly from a DEVICE-RESIDENT feature store (a split's clips packed into store [rows, E] fp32, clip i =
 * rows offsets[i] .. offsets[i+1]): out[b, t, :] = store[offsets[idx[b]] + t] for t < len(clip idx[b]), else 0;
 * mask[b, t] = 1 where padded.  out: [B, Tmax, E] of out_dtype (fp32, or bf16 = the encoder's compute type, which
 * saves its input cast), mask: uint8/bool [B, Tmax].  E % 4 == 0 takes the 16-byte path.
 * replaces: per-sample np.load + torch.tensor (dataloader.py:378-386), zero-pad + mask build on the host
 * (_make_mask_video, dataloader.py:233-247) and the per-step H2D copies (train.py:120-121).
 * --------------------------------------------------------------------------------------------- */
int vct_gather_pad_rows(int out_dtype, int B, int Tmax, int E, const float* store, const int64_t* offsets,
                        const int64_t* idx, void* out, uint8_t* mask, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Fused Adam / AdamW step over the flat fp32 parameter buffer + bf16 shadow refresh, one launch.
 * replaces: torch.optim.Adam(...).step() / AdamW when weight_decay != 0 (train.py:24-31,126); same
 * arithmetic as torch's single-tensor Adam (no amsgrad).  step_dev: DEVICE int32 counter of steps
 * already taken (read for the bias corrections, then incremented by a 1-thread kernel).
 * shadow_bf16 may be NULL; elements [shadow_skip_begin, shadow_skip_end) get no shadow (the token
 * embedding is gathered from the fp32 master; offsets relative to `param`).  n must be a multiple of 4.
 * A step may be applied range by range (each range as soon as its gradients are final, on a side stream):
 * pass bump_step = 0 for all ranges and finish with one call n = 0, bump_step = 1.
 * hyper_dev: optional DEVICE fp32 [5] = {lr, beta1, beta2, eps, weight_decay}; when given it overrides the scalar
 * arguments, so a captured graph / recorded launch list follows an LR schedule (scalars are frozen at record time).
 * --------------------------------------------------------------------------------------------- */
int vct_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, void* shadow_bf16,
                  int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay,
                  int32_t* step_dev, int64_t shadow_skip_begin, int64_t shadow_skip_end, int32_t bump_step,
                  const float* hyper_dev, void* stream);
/* The same step over ONE 2-D weight [rows, cols] (cols a multiple of 64; contiguous) that also writes its TRANSPOSED bf16 shadow
 * shadow_t [cols][ld_t >= rows] -- W_g^T for the NT form of the vocabulary dX -- in the same pass (no step-counter bump). */
/* vct_adam_step that ALSO writes the stream-order packed copies (vct_ss_pack layout) of the weight matrices listed in segs_dev
 * (device array, sorted by `begin`; flat element indices of the WHOLE parameter buffer, `base` = index of param[0] in it):
 * mode 0 = the matrix [N, K] is packed as 512-row blocks, block i at chunk chunk0[i]; mode 1 = a 512-row matrix packed as 512-column
 * K slices, slice i at chunk0[i] (chunk0 < 0: not packed).  No reference counterpart (a layout copy refreshed with the shadow). */
typedef struct vct_adam_pack_seg { int64_t begin, end; int32_t K, mode; int32_t chunk0[4]; void* stream; } vct_adam_pack_seg;
int vct_adam_step_pk(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, void* shadow_bf16,
                     int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay,
                     int32_t* step_dev, int64_t shadow_skip_begin, int64_t shadow_skip_end, int32_t bump_step,
                     const float* hyper_dev, const vct_adam_pack_seg* segs_dev, int32_t nseg, int64_t base, void* stream);
/* The same step over a LIST of flat ranges in ONE launch -- what is left for a separate pass when the weight matrices are stepped by
 * the optimizer epilogue of their own weight-gradient GEMMs (vct_gemm_adam): biases, LayerNorm parameters, the token-embedding table.
 * param / grad / exp_avg / exp_avg_sq / shadow_bf16: the WHOLE flat buffers; ranges_dev: device array sorted by begin, [begin, end)
 * flat elements (multiples of 4), blk0 = number of 4096-element workgroups of all earlier ranges, shadow != 0: write the bf16 shadow
 * (and the packed copies of segs_dev, flat indices as in vct_adam_step_pk with base 0); total_blocks = workgroups of all ranges.
 * No step-counter bump.  replaces torch.optim.Adam.step (train.py:24-26,126) for those parameters. */
typedef struct vct_adam_range { int64_t begin, end; int32_t blk0, shadow; } vct_adam_range;
int vct_adam_step_ranges(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, void* shadow_bf16,
                         const vct_adam_range* ranges_dev, int32_t nranges, int32_t total_blocks, float lr, float beta1, float beta2,
                         float eps, float weight_decay, int32_t* step_dev, const float* hyper_dev,
                         const vct_adam_pack_seg* segs_dev, int32_t nseg, void* stream);
/* vct_adam_step_ranges with an optional per-range row table: rows_dev (device array of nranges entries, or NULL) says for range i
 * that it lies inside a row-major table whose row 0 starts at flat element `origin`, rows of row_len elements (a multiple of 4),
 * nrows rows, and live[r] != 0 for every row that has ever had a non-zero gradient or moment (vct_embed_bwd_live /
 * vct_embed_live_rebuild keep that true).  A row that is not live is neither read nor written: with g = m = v = 0 the update
 * changes nothing, bit for bit, PROVIDED 1 - lr * weight_decay == 1, eps > 0 and the step size is finite -- checked by the kernel
 * on the hyper-parameters it reads (hyper_dev when given) in a form that needs no pow(): 0 <= lr <= 1e30, 0 <= beta1 <= 0.9999,
 * 0 <= beta2 <= 0.99999, eps finite; otherwise the range is stepped densely.  live == NULL, a range with a shadow, or a row_len
 * that is no multiple of 4: dense.  Elements of the range in front of `origin` or behind row nrows - 1
 * (alignment padding) are stepped.  Live rows get the bits of vct_adam_step_ranges. */
typedef struct vct_adam_rows { int64_t origin; int32_t row_len, nrows; const uint8_t* live; } vct_adam_rows;
int vct_adam_step_ranges_rows(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, void* shadow_bf16,
                              const vct_adam_range* ranges_dev, int32_t nranges, int32_t total_blocks, float lr, float beta1, float beta2,
                              float eps, float weight_decay, int32_t* step_dev, const float* hyper_dev,
                              const vct_adam_pack_seg* segs_dev, int32_t nseg, const vct_adam_rows* rows_dev, void* stream);
int vct_adam_step_2d(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, void* shadow_bf16,
                     void* shadow_t_bf16, int32_t rows, int32_t cols, int64_t ld_t, float lr, float beta1, float beta2,
                     float eps, float weight_decay, int32_t* step_dev, const float* hyper_dev, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Gradient clipping over the flat fp32 gradient buffer (csrc/vct_grad_clip.hip).
 * replaces: torch.nn.utils.clip_grad_norm_ (L2, error_if_nonfinite = False) / torch.nn.utils.clip_grad_value_ on the parameters an
 * optimizer owns.  No reference counterpart in train.py (the reference never clips); the arithmetic is torch's:
 *   norm = || (||g_1||, ..., ||g_n||) ||_2, coef = clamp(max_norm / (norm + 1e-6), max = 1), g_i *= coef   |   g_i.clamp_(-v, v).
 * segs_dev: DEVICE table of nseg flat-element segments [begin, end), sorted and disjoint, one per parameter; begin a multiple of
 * 4, end arbitrary (the last elements of a segment are handled one by one: no reliance on padding, nothing outside a segment is read
 * or written); blk0 = number of 4096-element workgroups of all earlier segments (as vct_adam_range), total_blocks = those of all.
 * vct_grad_sqnorm (two launches, no atomics, two runs give the same bits): every element is widened to fp64 and accumulated by
 * fp64 FMAs, one partial per workgroup in a fixed order; then one workgroup adds the partials of each segment (a wave per segment,
 * fixed stride, fixed shuffle tree) and the segment sums in ascending order.
 *   partials : DEVICE fp64 [total_blocks + nseg] scratch (the workgroup partials, then the segment sums), 16-byte aligned
 *   seg_norm : DEVICE fp32 [nseg] <- (float)sqrt(sum_i)
 *   clip_dev : DEVICE fp32 [2] = {max_norm, max_value}; read by the kernels, so recordings follow a change
 *   state    : DEVICE fp32 [4] <- {norm = (float)sqrt(sum of the segment sums), coef, 0, 0} with, in fp32,
 *              q = max_norm / (norm + 1e-6f), coef = q > 1 ? 1 : q (a NaN stays, as with torch.clamp).
 * vct_grad_clip_apply (one launch, plain vector stores): mode 0 multiplies every element of every segment by state[1] -- a
 * workgroup that reads exactly 1.0f leaves without touching memory, which is bitwise the multiplication; mode 1 clamps to
 * [-clip_dev[1], clip_dev[1]] like torch.clamp (NaN stays NaN, -0.0 stays -0.0; state may be NULL).
 * Null pointers: VCT_E_ARG; nseg <= 0 or total_blocks <= 0: VCT_E_SHAPE; grad / partials / segs_dev not 16-byte aligned: VCT_E_ALIGN.
 * --------------------------------------------------------------------------------------------- */
typedef struct vct_grad_seg { int64_t begin, end; int32_t blk0, reserved; } vct_grad_seg;
int vct_grad_sqnorm(const float* grad, const vct_grad_seg* segs_dev, int32_t nseg, int32_t total_blocks, double* partials,
                    float* seg_norm, const float* clip_dev, float* state, void* stream);
int vct_grad_clip_apply(float* grad, const vct_grad_seg* segs_dev, int32_t nseg, int32_t total_blocks, int32_t mode,
                        const float* clip_dev, const float* state, void* stream);

/* elementwise helpers ------------------------------------------------------------------------ */
/* dst[i] = (dst_dtype) src[i], n elements (fp32 <-> bf16 parameter / feature casts) */
int vct_cast(int src_dtype, int dst_dtype, const void* src, void* dst, int64_t n, void* stream);
/* read-only pass over `bytes` bytes at src (16-byte aligned): brings a buffer that the NEXT launch streams (the packed weight streams
 * of the sample-stationary stacks, whose first touch is otherwise an HBM miss per chunk) into the memory-side cache.  No reference
 * counterpart (cache placement). */
int vct_warm(const void* src, int64_t bytes, void* stream);
/* first-index argmax per row (torch.max(dim=1) tie-break, MMT4Caption.py:165); out[row * out_stride] int64
 * (out_stride lets the decode loop write straight into column t of the id matrix ys[B, max_len]) */
/* dst[c, r] = src[r, c] (bf16 only): the transposed shadow of the vocabulary projection's weight, so that the input gradient
 * dX = dlogits W_g runs in the K-contiguous NT form (replaces nothing in the reference: autograd's `grad_output.mm(weight)`,
 * torch F.linear backward, reads W_g row-major). */
int vct_transpose(int dtype, int rows, int cols, const void* src, int64_t ld_src, void* dst, int64_t ld_dst, void* stream);
int vct_argmax_rows(int dtype, int rows, int cols, const void* x, int64_t ldx, int64_t* out, int64_t out_stride,
                    void* stream);
/* one greedy-decode selection step: vct_argmax_rows into column t of the id matrix PLUS the loop's end bookkeeping
 * (MMT4Caption.py:166-171) on the device: ended[row] (uint8, sticky) is set when the row emits end_id; ended_count
 * counts such rows; the row that completes the set stores t into all_ended_at[0] (atomic min).  Integer atomics
 * only.  The host reads all_ended_at every few steps instead of syncing per token (`.tolist()`, MMT4Caption.py:168).
 * Before a decode: ended = 0, ended_count = 0, all_ended_at = max_len. */
int vct_greedy_select(int dtype, int rows, int cols, const void* x, int64_t ldx, int64_t* out, int64_t out_stride,
                      int64_t end_id, uint8_t* ended, int32_t* ended_count, int64_t* all_ended_at, int32_t t,
                      void* stream);
/* ---------------------------------------------------------------------------------------------
 * Beam search on the KV-cached decode step (csrc/vct_beam.hip).
 * replaces: MMT4Caption.beam_decode (MMT4Caption.py:186, `pass` in the reference) and predict_video.py:170's `--beam N`
 * ("not support yet").  Semantics: decode.beam_decode_ids (fixed-width beams, finished hypotheses frozen).
 *
 * vct_beam_select: one selection step for B videos of K beams (1 <= K <= 16, K <= V; rows b*K .. b*K+K-1 of x are video b).
 *   x [B*K, ldx] bf16 / fp32 logits (V valid columns, ldx >= V); scores fp32 [B*K] and finished uint8 [B*K] are read and
 *   rewritten in place; parent int32 [B*K] receives the parent ROW (b*K + k) of every new slot; out[row * out_stride] (int64,
 *   column t of the token table) the appended token (pad_id for a finished parent).  finished_count: this step's int32
 *   counter (zero before the call); the call whose videos complete the set of B*K finished slots stores t into
 *   all_finished_at[0] (atomic min).  Two launches.  workspace: >= B*K*CH*(2 + 2K)*4 bytes, CH = ceil(V / (256 * (16 /
 *   sizeof(dtype))))  (else VCT_E_WORKSPACE).
 * vct_beam_reorder: for every layer l < L, row j < M and slot s < t: dst[l][j*Lmax + s][d:3d] = src[l][parent[j]*Lmax + s][d:3d]
 *   (cache rows of 3d elements, layer l at element offset l * layer_stride; src != dst: the other cache of a ping-pong pair).
 *   One launch. */
int vct_beam_select(int dtype, int B, int K, int V, const void* x, int64_t ldx, float* scores, uint8_t* finished,
                    int32_t* parent, int64_t* out, int64_t out_stride, int64_t end_id, int64_t pad_id,
                    int32_t* finished_count, int64_t* all_finished_at, int32_t t, void* workspace, int64_t workspace_bytes,
                    void* stream);
int vct_beam_reorder(int dtype, int L, int M, int Lmax, int d, int t, const int32_t* parent, const void* src, void* dst,
                     int64_t layer_stride, void* stream);
/* ---------------------------------------------------------------------------------------------
 * Sampled decoding on the KV-cached decode step (csrc/vct_sample.hip).  The reference has no sampling decoder; the semantics
 * are the project's (decode.sample_decode_ids).
 *
 * vct_sample_select: one selection step for `rows` independent rows: draws one token per row from the softmax of
 * x * inv_temp over the row's candidates and keeps vct_greedy_select's end bookkeeping.  The settings are READ FROM DEVICE
 * MEMORY (ctl, 16 bytes, 16-byte aligned), so one captured graph serves every seed / temperature / k / p:
 *   ctl = { uint32 seed; int32 top_k; float inv_temp; float top_p }      top_k is clamped to [0, min(64, V)] by the kernel
 * Per row r (x [rows, ldx] bf16 / fp32 logits, V valid columns, ldx >= V):
 *   ended[r] != 0 before the call: out = pad_id, step_logp = 0, seq_logp and the counters untouched.
 *   candidates  top_k == 0: all V tokens in index order; top_k >= 1: the min(top_k, V) largest RAW logits in rank order
 *               (value descending, ties to the smaller index).
 *   weights     z = float(x) * inv_temp (fp32), m = max z over the candidates, w = exp(z - m).
 *   nucleus     top_k >= 1 and top_p < 1: the shortest rank-order prefix whose running fp32 sum of w is >= top_p * (sum of
 *               every candidate's w); at least one candidate is kept.
 *   draw        W = sum of the kept w; the first kept candidate, in candidate order, whose running sum exceeds u * W (the
 *               last kept one if rounding leaves none); u = (h >> 8) * 2^-24, h = hash32(hash32(key) + (t * rows + r) *
 *               0x9E3779B1), key = (seed * 0x9E3779B1) ^ (997 * 0x85EBCA77 + 0x165667B1), all in uint32 (the dropout
 *               kernels' counter hash at site 997).
 *   outputs     out[r * out_stride] (int64, column t of the id table) = the token; step_logp[r] = z_c - m - log(W), the
 *               log-probability under the distribution sampled from; seq_logp[r] += step_logp[r] (one writer per row);
 *               token == end_id: ended / ended_count / all_ended_at exactly as vct_greedy_select.
 * Two launches, fixed-order reductions, no floating-point atomics: a second call on the same inputs is bit-identical.
 * workspace: 16-byte aligned, >= vct_sample_select_workspace_bytes(dtype, rows, V) = rows * CH * (2 + 2 * 64) * 4 bytes,
 * CH = ceil(V / (256 * (16 / sizeof(dtype)))) (sized for the largest k; else VCT_E_WORKSPACE; 0 for a bad argument).
 * --------------------------------------------------------------------------------------------- */
typedef struct vct_sample_ctl {
  uint32_t seed;
  int32_t top_k;
  float inv_temp;
  float top_p;
} vct_sample_ctl;

typedef struct vct_sample_select_desc {
  int32_t dtype;              /* VCT_F32 / VCT_BF16: the logits */
  int32_t rows, V, t;
  const void* x;
  int64_t ldx;
  int64_t* out;
  int64_t out_stride;
  int64_t end_id, pad_id;
  uint8_t* ended;             /* [rows], sticky */
  int32_t* ended_count;
  int64_t* all_ended_at;
  float* step_logp;           /* [rows], written */
  float* seq_logp;            /* [rows], += */
  const vct_sample_ctl* ctl;  /* device memory */
  void* workspace;
  int64_t workspace_bytes;
} vct_sample_select_desc;

int64_t vct_sample_select_workspace_bytes(int dtype, int rows, int V);
int vct_sample_select(const vct_sample_select_desc* d, void* stream);
/* ---------------------------------------------------------------------------------------------
 * Generation controls on the KV-cached decode step (csrc/vct_logit_controls.hip).  The reference has no logit rule of any kind;
 * the semantics are the project's (decode.GenerationControls) and follow Hugging Face's logits processors of the same names.
 *
 * vct_logit_controls: edits the logits of step t IN PLACE, in their dtype, columns < V only, for `rows` rows, in front of the
 * selection kernel of that step.  The settings are READ FROM DEVICE MEMORY (ctl, 160 bytes), so one captured graph serves every
 * setting:
 *   ctl = { int32 min_length; int32 ngram; float theta; float inv_theta; int32 n_banned; int32 reserved[3]; int32 banned[32] }
 *   ngram is clamped to [0, 8] and n_banned to [0, 32] by the kernel; a banned id or history token outside [0, V) is ignored.
 * History of row r: h[0 .. t-1].  parents == NULL: h[s] = ids[r * ids_stride + s] (the id matrix of a greedy / sampled session).
 * parents != NULL (beams, rows = B*K, rows b*K .. b*K+K-1 = video b): ids is the token table and h follows the parent
 * back-track as of step t: j = r; for s = t-1 .. 1: h[s] = ids[j * ids_stride + s], j = parents[s * parents_stride + j];
 * h[0] = ids[j * ids_stride] (a parent outside its video's K rows is clamped into them).
 * Per row with ended[r] == 0 (a row with ended[r] != 0 is not touched):
 *   1. penalty  theta != 1: for every distinct token v of h that rule 2 does not ban, once: f = float(x[v]);
 *               x[v] = round-to-nearest-even(f > 0 ? f * inv_theta : f * theta).
 *   2. bans     x[v] = -inf for every banned[i], i < n_banned; for end_id while t <= min_length; and, with n = ngram >= 1 and
 *               t >= n-1, for every h[j], n-1 <= j <= t-1, whose n-1 predecessors h[j-n+1 .. j-1] equal h[t-n+1 .. t-1].
 * No element is written twice with different values.  One launch: a wave per row (four rows per workgroup), or with parents a
 * workgroup per video and a wave per slot over the video's parent / token columns staged in LDS.  No atomics, no workspace; a
 * second call on the same inputs is bit-identical.
 * VCT_E_ARG: NULL descriptor / x / ids / ended / ctl, bad dtype; VCT_E_SHAPE: rows <= 0, V <= 0, ldx < V, t < 1, t > 64, and with
 * parents K outside 1 .. 16 or rows not a multiple of K.  All before any device use.
 * --------------------------------------------------------------------------------------------- */
typedef struct vct_logit_ctl {
  int32_t min_length;
  int32_t ngram;
  float theta;
  float inv_theta;
  int32_t n_banned;
  int32_t reserved[3];
  int32_t banned[32];
} vct_logit_ctl;

typedef struct vct_logit_controls_desc {
  int32_t dtype;              /* VCT_F32 / VCT_BF16: the logits */
  int32_t rows, V, t;
  void* x;                    /* [rows, ldx], edited in place */
  int64_t ldx;
  int64_t end_id;
  const int64_t* ids;         /* id matrix, or the beams' token table */
  int64_t ids_stride;
  const uint8_t* ended;       /* [rows]: the session's ended / finished flags */
  const int32_t* parents;     /* beams: [Lmax, rows] parent rows; NULL: histories are the rows of ids */
  int64_t parents_stride;
  int32_t K;                  /* beams per video (with parents) */
  int32_t reserved;
  const vct_logit_ctl* ctl;   /* device memory */
} vct_logit_controls_desc;

int vct_logit_controls(const vct_logit_controls_desc* d, void* stream);
/* ---------------------------------------------------------------------------------------------
 * Ensemble decoding (csrc/vct_ensemble.hip).  The reference decodes with one checkpoint; the semantics are the project's
 * (decode.Ensemble): the next-token distributions of n models are averaged at every step, and the result is handed to the
 * controls and selection kernels above as one fp32 row of log-probabilities (a row of log-probabilities is a valid logits row).
 *
 * vct_ensemble_combine: per row r and member m (fp32 throughout): z = float(x_m[r, v]), M_m = max_v z, S_m = sum_v exp(z - M_m),
 * lp_m[v] = (z - M_m) - log S_m over the columns [0, V).  The weights w are READ FROM DEVICE MEMORY (fp32 [VCT_ENSEMBLE_MAX], the
 * host normalises them: w_m >= 0, sum 1), so one captured graph serves every weighting.  A member with w_m == 0 (or a w_m that
 * is not > 0) is skipped altogether -- not multiplied, so 0 * -inf cannot appear -- and none of its memory is read.
 *   VCT_ENS_LOGP   out[r, v] = sum_m w_m lp_m[v], accumulated in member order (the geometric mean; the selection renormalises)
 *   VCT_ENS_PROB   A = max over the members with w_m > 0 of lp_m[v];  out[r, v] = A + log sum_m w_m exp(lp_m[v] - A), -inf when
 *                  A is -inf (the arithmetic mean of the probabilities)
 * NaN in a member's row makes that row of out NaN and no other.  Columns >= V of x_m and of out are neither read nor written.
 * One launch, one workgroup per row, three sweeps over each member's row (max, sum, combination: the second and third are served
 * by the caches); 16-byte loads and stores where a tensor's base and row stride keep rows 16-byte aligned, element accesses
 * otherwise and for the V % 8 tail.  Fixed-order reductions, no atomics, no workspace: a second call is bit-identical.
 * VCT_E_ARG: NULL descriptor / x_m / w / out, bad dtype or mode; VCT_E_SHAPE: n outside 1 .. VCT_ENSEMBLE_MAX, rows < 1, V < 1,
 * ld_m < V, ld_out < V.  All before any device use.
 * --------------------------------------------------------------------------------------------- */
#define VCT_ENSEMBLE_MAX 8
enum { VCT_ENS_PROB = 0, VCT_ENS_LOGP = 1 };
typedef struct vct_ensemble_desc {
  int32_t n, mode, rows, V;                 /* members 1..8; columns [0, V) are read and written */
  int32_t dtype[VCT_ENSEMBLE_MAX];          /* VCT_F32 | VCT_BF16 per member */
  const void* x[VCT_ENSEMBLE_MAX];          /* member logits [rows, ld_m] */
  int64_t ld[VCT_ENSEMBLE_MAX];
  const float* w;                           /* DEVICE fp32 [VCT_ENSEMBLE_MAX]: w_m >= 0, sum 1 */
  float* out;                               /* fp32 [rows, ld_out] */
  int64_t ld_out;
} vct_ensemble_desc;

int vct_ensemble_combine(const vct_ensemble_desc* d, void* stream);
/* ---------------------------------------------------------------------------------------------
 * One stage of the greedy-decode step at SMALL batch (B <= 4): out[b, n] = epilogue(W[n, :] . prologue(...)[b, :]), a weight-
 * streaming matrix-vector kernel whose prologue builds the input vector and whose epilogue finishes the stage, so that the
 * embedding / LayerNorm / attention launches of the per-token step vanish into their consumers (csrc/vct_decode.hip):
 *   pro = VCT_DEC_PRO_NONE        x = x_in[b, 0:K)                                  (fp32)
 *         VCT_DEC_PRO_EMBED       x = table[ids[b*id_stride], :] + pos_row          (nn.Embedding + PositionalEmbedding, CapDecoder.py:64-66)
 *         VCT_DEC_PRO_LN          x = LayerNorm(x_in; g1, b1)                       (the previous stage stored the PRE-norm sum)
 *         VCT_DEC_PRO_LN_LN       x = LayerNorm(LayerNorm(x_in; g1, b1); g2, b2)    (last layer's norm3, then decoder.norm)
 *         VCT_DEC_PRO_SELF_ATTN / _CROSS_ATTN   x = MHA core of ONE query per batch row: q [B] rows (stride q_bs), keys / values
 *                                 kc / vc + b*kv_bs + l*kv_ld for l < Lk (<= 64), H heads of K/H columns; no mask (CapDecoder.py:70-75:
 *                                 the newest token attends to every cached position)
 *   epilogue: + bias[n], act, + res[b*ld_res + n] (fp32), stored as fp32 or -- out_native -- in the weight dtype (q|k|v into the KV-cache
 *   slot, logits).  x_out (optional, fp32 [B, K]): the prologue's vector, written once (the next stage's residual).
 *   W: [N, K] row-major, wdtype VCT_BF16 (K % 512 == 0) or VCT_F32 (K % 256 == 0), K <= 2048; KV cache and q in the same dtype.
 * replaces: per token and decoder layer, self_attn / multihead_attn (in_proj, SDPA, out_proj), linear1 / linear2, norm1-3 of
 * nn.TransformerDecoderLayer (torch nn/modules/transformer.py:1143-1199) as called from CapDecoder.decode_word (CapDecoder.py:62-79),
 * plus decoder.norm and the generator: 6 launches per layer + 1 instead of 11 + 2.
 * --------------------------------------------------------------------------------------------- */
enum { VCT_DEC_PRO_NONE = 0, VCT_DEC_PRO_EMBED = 1, VCT_DEC_PRO_LN = 2, VCT_DEC_PRO_LN_LN = 3, VCT_DEC_PRO_SELF_ATTN = 4,
       VCT_DEC_PRO_CROSS_ATTN = 5 };
typedef struct vct_decode_gemv_desc {
  int32_t wdtype, B, N, K;
  const void* W; int64_t ldw;
  const float* bias;
  int32_t pro, act;
  const float* x_in; int64_t ld_x;
  const float* g1; const float* b1; const float* g2; const float* b2;
  const int64_t* ids; int64_t id_stride; const float* table; const float* pos_row;
  const void* q; int64_t q_bs; const void* kc; const void* vc; int64_t kv_ld, kv_bs; int32_t H, Lk;
  const float* res; int64_t ld_res;
  void* out; int64_t ld_out; int32_t out_native; int32_t rows_per_wave;   /* rows_per_wave: 0 = auto */
  float* x_out;
} vct_decode_gemv_desc;
int vct_decode_gemv(const vct_decode_gemv_desc* d, void* stream);

/* ---------------------------------------------------------------------------------------------
 * One nn.Linear of the greedy-decode step at LARGER batch (2 <= M = captions in flight <= 256), applied to the M rows of the
 * current position:  out[M, N] = act(in W^T + bias) + res,  W bf16 [N, K] row-major (csrc/vct_gemm_skinny.hip: MFMA fragments
 * straight from L2, K split over the eight waves of a workgroup, 16 output columns per workgroup).  Input, one of
 *   x      bf16 rows (ldx)                                                    -- or --
 *   x_pre  fp32 PRE-norm rows: in = LayerNorm(x_pre; ln_g, ln_b, eps 1e-5), normalised in registers (K <= 1024); with x_norm
 *          the normalised rows are also stored (fp32, once) for the residual of a later call.  With ids (int64, row r at
 *          ids[r * id_stride]) the rows are instead EMBEDDED: in = x_pre[ids[r]] + ln_b, x_pre = the fp32 table [V, K] and ln_b the
 *          positional row (nn.Embedding + PositionalEmbedding, CapDecoder.py:64-66); ln_g is not read.
 * res: rows of res_dtype (VCT_F32 or VCT_BF16) added after the activation.  out: bf16 or fp32 rows (ldo: e.g. a KV-cache slot).
 * K % 8 == 0; pointers 16-byte aligned, leading dimensions multiples of 8 (bf16) / 4 (fp32).
 * replaces: norm1 / norm2 / norm3 + the Linear that consumes them, and the `x + sublayer(x)` adds, of nn.TransformerDecoderLayer
 * (torch nn/modules/transformer.py:1143-1199) as called per token from CapDecoder.decode_word (CapDecoder.py:62-79): 8 launches per
 * layer instead of 11.
 * --------------------------------------------------------------------------------------------- */
typedef struct vct_decode_linear_desc {
  int32_t M, N, K;
  int32_t out_dtype, act, res_dtype;
  const void* x; int64_t ldx;
  const float* x_pre; int64_t ld_pre;
  const float* ln_g; const float* ln_b;
  float* x_norm; int64_t ld_norm;
  const void* W; int64_t ldw;
  const float* bias;
  const void* res; int64_t ld_res;
  void* out; int64_t ldo;
  const int64_t* ids; int64_t id_stride;
} vct_decode_linear_desc;
int vct_decode_linear(const vct_decode_linear_desc* d, void* stream);
/* y[M, K] (bf16) = LayerNorm(LayerNorm(x; g1, b1); g2, b2) of fp32 rows (g2 = b2 = NULL: one LayerNorm): the last layer's norm3
 * followed by decoder.norm (CapDecoder.py:20) in front of the generator.  K <= 1024, K % 4 == 0. */
int vct_decode_ln2(int M, int K, const float* x, int64_t ldx, const float* g1, const float* b1, const float* g2, const float* b2,
                   void* y, int64_t ldy, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Batch-1 greedy-decode step, one launch per BLOCK of a decoder layer (csrc/vct_decode_block.hip; bf16 weights, fp32 vectors):
 *   kind 0  self-attention block   x -> q|k|v of the new token (-> cache slot), attention over Lk cached keys (the last one is
 *                                  the new token), PARTIAL out-projection per head: part_out[h][d]
 *   kind 1  cross-attention block  x1 -> q, attention over the memory's Lk cached K/V rows, partial out-projection per head
 *   kind 2  feed-forward block     x2 -> act(W1 x2 + b1) per 64 hidden units, partial linear2 per unit group: part_out[ff/64][d]
 *   kind 3  generator              y -> logits fp32 [V] (part_out) (+ the greedy selection of the token, see sel_ws)
 * The input vector of every launch is built by each workgroup: the embedded token (id / table / pos_row) or
 * res + res_bias + sum_c part[c] (the previous block's residual, the bias of its second product, its partial vectors),
 * followed by LayerNorm(g1, b1) and LayerNorm(g2, b2) when given; x_out receives it (the next block's residual).
 * res is REQUIRED whenever id is absent (res_bias and part stay optional; part alone is VCT_E_ARG): the kernels load it
 * unconditionally.  res, res_bias, part, table and pos_row are read as 16-byte vectors: one that is given and not 16-byte
 * aligned is VCT_E_ALIGN.  n_part <= 32 partial vectors (else VCT_E_SHAPE); g2 / b2 only together with g1 / b1.
 * replaces: CapDecoder.decode_word for one caption (model/CapDecoder.py:62-79; torch nn/modules/transformer.py:1143-1199) --
 * 3 launches per layer instead of the 6 of vct_decode_gemv.  w_a / b_a: the first product's weight rows [*, d] and bias
 * (in_proj | q rows | linear1 | generator); w_b: the second product's weight TRANSPOSED, [*, d] = [in, out] (out_proj^T |
 * linear2^T: a workgroup's 64 input columns are then 64 contiguous rows).
 * vct_decode_block_supported: bf16, d = 512 with head_dim 64 (8 heads), ff a multiple of 64 (<= 2048), Lk <= 64.
 * --------------------------------------------------------------------------------------------- */
typedef struct vct_decode_block_desc {
  int32_t kind, d, ff, V, Lk, act;
  const int64_t* id; const float* table; const float* pos_row;
  const float* res; const float* res_bias; const float* part; int32_t n_part, pad0;
  const float* g1; const float* b1; const float* g2; const float* b2;
  float* x_out;
  const void* w_a; int64_t ld_a; const float* b_a;
  void* slot;
  const void* kc; const void* vc; int64_t kv_ld;
  const void* w_b; int64_t ld_b;
  float* part_out;
  /* kind 3 only, optional (sel_ws != NULL): the greedy selection of vct_greedy_select for this ONE caption inside the generator
   * launch -- every workgroup leaves its (max, first index) pair in sel_ws (fp32 [2 * ceil(V / 128) + 1], 8-byte aligned (else VCT_E_ALIGN), zero-initialised once:
   * the last word is a ticket counter the launch leaves at zero), the last one to finish writes tok_out[0] and the end-of-sequence
   * bookkeeping (ended[0], ended_count, all_ended_at = min(., t)). */
  float* sel_ws; int64_t* tok_out; int64_t end_id; uint8_t* ended; int32_t* ended_count; int64_t* all_ended_at; int32_t t, pad1;
} vct_decode_block_desc;
int vct_decode_block_supported(int dtype, int d, int H, int ff, int Lk);
int vct_decode_block(const vct_decode_block_desc* d, void* stream);

/* seed[0] += 1 (one-thread kernel, keeps the dropout stream advancing inside a captured graph) */
int vct_advance_seed(uint32_t* seed, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Host runtime: recorded launch lists, cross-stream ordering, live kernel timing (csrc/vct_runtime.hip).
 * replaces: the Python interpreter + torch dispatcher that issue the reference's step op by op (train.py:119-131);
 * there is no counterpart object in the reference.
 *
 * Launch list: between vct_cmdlist_begin and vct_cmdlist_end every vct_* call made ON THIS HOST THREAD is validated
 * and planned as usual but its kernel launches (and memsets, sync points, taps) are RECORDED instead of executed --
 * kernel, geometry, by-value argument copies and the stream they were aimed at.  vct_cmdlist_replay re-issues them in
 * the recorded order with eager semantics: launches aimed at `main_stream` of _begin go to `main_stream` of _replay,
 * every other stream is used as recorded (the caller keeps those streams alive).  Device pointers are baked: record
 * against static buffers.  A list is not thread safe; one recording per thread at a time.
 * --------------------------------------------------------------------------------------------- */
int vct_cmdlist_create(void** out_list);
int vct_cmdlist_destroy(void* list);
int vct_cmdlist_begin(void* list, void* main_stream);
int vct_cmdlist_end(void* list);
int vct_cmdlist_replay(void* list, void* main_stream);
int vct_cmdlist_size(void* list);     /* recorded commands */
int vct_cmdlist_streams(void* list);  /* distinct streams seen while recording */
/* A replayed command cannot hand a status back to the call that recorded it: the FIRST non-zero status any command of a
 * replay produces (a failed RCCL collective: ncclResult_t + 10000; a failed event record / wait / memset: hipError_t) is
 * kept and returned by that vct_cmdlist_replay.  vct_cmdlist_inject_status is the fault-injection hook of that path:
 * eager it returns `status`; while recording it appends a command on `stream` that reports `status` at every replay. */
int vct_cmdlist_inject_status(int status, void* stream);
/* Host work in launch order: fn(arg) runs on the calling host thread after everything enqueued on `stream` so far has
 * FINISHED (the stream is synchronised first) -- now, or at that point of every replay while recording.  A non-zero return
 * of fn is reported like any other command status.  For collectives that are host calls (gloo / torch.distributed in the
 * one-GPU multi-rank tests); RCCL collectives (vct_comm_*) are stream work and never need it. */
int vct_cmdlist_host_call(int (*fn)(void*), void* arg, void* stream);
/* Cross-stream ordering, recordable: `waiter` will not run work enqueued after this call before everything enqueued on
 * `signal` so far has finished (event record + stream wait; replaces torch's Stream.wait_stream on the fast path). */
int vct_stream_wait(void* waiter_stream, void* signal_stream);
/* Named sync points 0..63: vct_sync_record marks "everything enqueued on `stream` so far"; a later vct_sync_wait on any
 * stream waits for the most recent mark with that id. */
int vct_sync_record(int id, void* stream);
int vct_sync_wait(int id, void* stream);
/* ---------------------------------------------------------------------------------------------
 * Gradient exchange over RCCL / xGMI (csrc/vct_comm.hip).  One communicator per process (one process per GPU).
 * replaces: DistributedDataParallel's bucketed NCCL all-reduce (train.py:217-219, utils.py:137-146).
 *   vct_comm_unique_id: rank 0 fills 128 bytes; the caller ships them to every rank (any side channel).
 *   vct_comm_init: collective over all ranks; the communicator owns a HIP stream for its collectives.
 *   Collectives are IN PLACE on device buffers and asynchronous: enqueued on the communicator's stream, ordered behind
 *   everything enqueued so far on after_stream when order_after != 0 (after_stream may be the NULL stream):
 *     vct_comm_allreduce_avg       buf[0:count)              <- mean over ranks
 *     vct_comm_reduce_scatter_avg  buf[r*n : (r+1)*n)        <- mean over ranks of that slice (n = count_per_rank, r = own rank)
 *     vct_comm_all_gather          buf[q*n : (q+1)*n)        <- rank q's slice, for every q
 *     vct_comm_broadcast           buf[0:count)              <- root's
 *   dtype VCT_F32 | VCT_BF16.  vct_comm_wait(comm, s): stream s waits for everything issued on the communicator so far.
 *   vct_comm_stream: the communicator's stream (to enqueue the optimizer of an owned shard between a reduce-scatter and
 *   the all-gather of its result).  All of these are recordable into launch lists.
 *   Return codes >= 10000 are ncclResult_t + 10000.  vct_comm_available() == 0: no RCCL could be bound at run time.
 * --------------------------------------------------------------------------------------------- */
int vct_comm_available(void);
int vct_comm_unique_id(uint8_t* out128);
int vct_comm_init(const uint8_t* id128, int rank, int world, void** out_comm);
int vct_comm_destroy(void* comm);
int vct_comm_rank(void* comm);
int vct_comm_world(void* comm);
int vct_comm_stream(void* comm, void** out_stream);
int vct_comm_allreduce_avg(void* comm, void* buf, int64_t count, int dtype, void* after_stream, int order_after);
int vct_comm_reduce_scatter_avg(void* comm, void* buf, int64_t count_per_rank, int dtype, void* after_stream, int order_after);
int vct_comm_all_gather(void* comm, void* buf, int64_t count_per_rank, int dtype, void* after_stream, int order_after);
int vct_comm_broadcast(void* comm, void* buf, int64_t count, int dtype, int root, void* after_stream, int order_after);
int vct_comm_wait(void* comm, void* stream);

/* A stream whose kernels may only run on the compute units set in cu_mask (bit i of word i/32 = CU i; `words` 32-bit
 * words; words == 0: an ordinary non-blocking stream).  MI355X has 256 CUs in 8 XCDs; a throughput-bound kernel (the
 * vocabulary weight gradient, Adam) confined to a subset of the CUs runs BESIDE a latency-bound chain of small kernels
 * confined to the complement instead of starving it (hipExtStreamCreateWithCUMask).  The caller owns the stream. */
int vct_stream_create_masked(const uint32_t* cu_mask, int words, void** out_stream);
int vct_stream_destroy(void* stream);
/* Live kernel timing with HIP events on the launch stream (bench.py's roofline block): vct_tap(tag, 0, s) / vct_tap(tag,
 * 1, s) bracket a region of stream s; every bracket executed (eagerly or by a replay) while taps are enabled adds one
 * (start, end) pair to tag's pool.  vct_tap_collect waits for the pairs, writes their elapsed milliseconds
 * (<= cap values) and resets the tag.  tag 0..15.  Disabled taps cost nothing and are not recorded. */
int vct_tap_enable(int on);
int vct_tap(int tag, int phase, void* stream);
int vct_tap_collect(int tag, float* ms_out, int cap);

#ifdef __cplusplus
}
#endif
#endif /* VCT_HIP_H */
