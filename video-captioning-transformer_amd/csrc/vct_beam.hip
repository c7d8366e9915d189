// Beam-search selection and KV-cache reorder for the KV-cached decode step on gfx950.
//
// replaces: MMT4Caption.beam_decode (reference model/MMT4Caption.py:186, a stub) and predict_video.py:170's `--beam N`
// ("not support yet").  The reference defines no semantics; the project's (decode.beam_decode_ids docstring) are:
// fixed-width beams with frozen finished hypotheses.  Per video b the K slots hold a score s and a finished flag; a step
// offers, for every unfinished slot k, the V candidates (k, v) valued s[k] + (logit[k, v] - logsumexp(logit[k, :V])) and, for
// every finished slot, the one candidate (k, pad_id) valued s[k]; the K best (ties: smaller flat index k * V + v) become the
// new slots in rank order.
//
// vct_beam_select, two launches:
//   stage 1  grid (V chunks, M = B * K rows), 256 threads: one 16-byte load per thread (a chunk is 256 x 16 bytes of a row) ->
//            the chunk's max, sum of exp(x - max), and its top K (logit, column), by K rounds of a workgroup arg-max over the
//            threads' remaining elements (shuffles, then one LDS exchange per round)
//   stage 2  one workgroup per video: logsumexp of each of its K rows from the chunk partials, then every partial top-K entry
//            (and the frozen candidate of each finished slot) through a per-thread sorted register list, K rounds of a
//            workgroup arg-max over the list heads, and the bookkeeping of the K winners.
// A row's contribution to the top K is among its own top-K logits: s[k] + (x - lse[k]) is monotone in x.  (Two distinct
// logits that round to the same value would be ranked by logit, not by flat index: the documented fp32 exception.)
// The two stages are two launches, so no inter-workgroup hand-off inside a launch: the partials reach stage 2 through the
// kernel boundary.  The tie rule, the chunk scan of stage 1, the arg-max reductions and the stop bookkeeping are
// vct_select_core.h's, shared with vct_select.hip and vct_sample.hip.
//
// vct_beam_reorder, one launch for every layer: slot s < t of row j of the other cache of a ping-pong pair <- slot s of row
// parent[j] (columns [d, 3d): k | v; q is only ever read at the current slot), whole 16-byte units where the row allows.
#include "vct_select_core.h"

namespace vct {

constexpr int BEAM_THREADS = SEL_THREADS;

template <typename T>
__global__ __launch_bounds__(BEAM_THREADS) void beam_partial_kernel(int V, int K, const T* __restrict__ x, int64_t ldx, bool vec_ok,
                                                                    float* __restrict__ pmax, float* __restrict__ psum,
                                                                    float* __restrict__ ptv, int* __restrict__ pti) {
  constexpr int VEC = 16 / (int)sizeof(T);
  __shared__ float s_v[2][SEL_WAVES];
  __shared__ int s_i[2][SEL_WAVES];
  __shared__ float s_sum[SEL_WAVES];
  const int chunk = blockIdx.x, CH = gridDim.x, row = blockIdx.y;
  float e[VEC];
  int id[VEC];
  sel_chunk_load<T, VEC>(x + (size_t)row * ldx, (chunk * BEAM_THREADS + threadIdx.x) * VEC, V, vec_ok, e, id);
  float hv, mv;
  int hi, mi;
  sel_head(e, id, hv, hi);
  mv = hv; mi = hi;
  sel_block_best<SEL_WAVES>(mv, mi, s_v, s_i, 0);
  // chunk max and sum of exp(x - max); a chunk without a finite logit sums to 0
  const float se = sel_chunk_expsum(e, id, 1.0f, mv, s_sum);
  const size_t pc = (size_t)row * CH + chunk;
  if (threadIdx.x == 0) { pmax[pc] = mv; psum[pc] = mv != -INFINITY ? se : 0.0f; }
  sel_chunk_topk(K, e, id, hv, hi, mv, mi, s_v, s_i, ptv, pti, pc, K);
}

// sorted (descending, ties by index) register list of a thread's best KMAX candidates; compile-time indices only
template <int KMAX>
struct BeamList {
  float v[KMAX];
  int i[KMAX];
  __device__ __forceinline__ void init() {
#pragma unroll
    for (int p = 0; p < KMAX; p++) { v[p] = -INFINITY; i[p] = SEL_NONE; }
  }
  __device__ __forceinline__ void insert(float nv, int ni) {
    if (!sel_better(nv, ni, v[KMAX - 1], i[KMAX - 1])) return;
    bool placed = false;
#pragma unroll
    for (int p = KMAX - 1; p > 0; p--) {
      if (!placed) {
        if (sel_better(nv, ni, v[p - 1], i[p - 1])) { v[p] = v[p - 1]; i[p] = i[p - 1]; }
        else { v[p] = nv; i[p] = ni; placed = true; }
      }
    }
    if (!placed) { v[0] = nv; i[0] = ni; }
  }
  __device__ __forceinline__ void pop() {
#pragma unroll
    for (int p = 0; p < KMAX - 1; p++) { v[p] = v[p + 1]; i[p] = i[p + 1]; }
    v[KMAX - 1] = -INFINITY; i[KMAX - 1] = SEL_NONE;
  }
};

template <int KMAX>
__global__ __launch_bounds__(BEAM_THREADS) void beam_merge_kernel(int K, int V, int CH, const float* __restrict__ pmax,
                                                                  const float* __restrict__ psum, const float* __restrict__ ptv,
                                                                  const int* __restrict__ pti, float* scores, uint8_t* finished,
                                                                  int32_t* __restrict__ parent, int64_t* __restrict__ out,
                                                                  int64_t out_stride, int64_t end_id, int pad_id, int M,
                                                                  int32_t* finished_count, unsigned long long* all_finished_at, int t) {
  __shared__ float s_lse[KMAX], s_s[KMAX];
  __shared__ uint8_t s_f[KMAX];
  __shared__ float s_wv[KMAX];
  __shared__ int s_wi[KMAX];
  __shared__ float s_v[2][SEL_WAVES];
  __shared__ int s_i[2][SEL_WAVES];
  const int b = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int row0 = b * K;
  if (threadIdx.x < K) {
    s_s[threadIdx.x] = scores[row0 + threadIdx.x];
    s_f[threadIdx.x] = finished[row0 + threadIdx.x];
  }
  // logsumexp of each row: one wave per row, lanes over the chunks, fixed reduction order
  for (int k = w; k < K; k += SEL_WAVES) {
    const size_t base = (size_t)(row0 + k) * CH;
    float m = -INFINITY;
    for (int c = lane; c < CH; c += 64) m = fmaxf(m, pmax[base + c]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    float s = 0.0f;
    if (m != -INFINITY)
      for (int c = lane; c < CH; c += 64) {
        const float pm = pmax[base + c];
        s += pm == -INFINITY ? 0.0f : psum[base + c] * expf(pm - m);
      }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) s_lse[k] = m == -INFINITY ? -INFINITY : m + logf(s);
  }
  __syncthreads();
  // candidates: every partial top-K entry of an unfinished row, the frozen (k, pad_id) of a finished one
  BeamList<KMAX> lst;
  lst.init();
  const int per_row = CH * K;
  for (int it = threadIdx.x; it < K * per_row; it += BEAM_THREADS) {
    const int k = it / per_row, j = it - k * per_row;
    if (s_f[k]) {
      if (j == 0) lst.insert(s_s[k], k * V + pad_id);
      continue;
    }
    const size_t e = (size_t)row0 * per_row + it;
    const int col = pti[e];
    if (col == SEL_NONE) continue;
    const float logp = ptv[e] - s_lse[k];
    lst.insert(s_s[k] + logp, k * V + col);
  }
  for (int r = 0; r < K; r++) {
    float bv = lst.v[0];
    int bi = lst.i[0];
    sel_block_best<SEL_WAVES>(bv, bi, s_v, s_i, r);
    if (bi == lst.i[0] && bi != SEL_NONE) lst.pop();
    if (threadIdx.x == 0) { s_wv[r] = bv; s_wi[r] = bi; }
  }
  __syncthreads();
  if (w == 0) {
    bool nf = false;
    if (lane < K) {
      const int flat = s_wi[lane];
      const int p = flat / V, v = flat - p * V;
      const int j = row0 + lane;
      nf = s_f[p] != 0 || (int64_t)v == end_id;
      parent[j] = row0 + p;
      out[(size_t)j * out_stride] = v;
      scores[j] = s_wv[lane];
      finished[j] = nf ? 1 : 0;
    }
    const int n = __popcll(__ballot(nf));
    if (lane == 0) sel_mark_ended(nullptr, n, finished_count, M, all_finished_at, t);   // the step's finished slots over all videos
  }
}

template <typename U>
__global__ __launch_bounds__(64) void beam_reorder_kernel(int M, int Lmax, int t, int64_t row_units, int64_t off_units,
                                                          int64_t n_units, int64_t layer_units, const int32_t* __restrict__ parent,
                                                          const U* __restrict__ src, U* __restrict__ dst) {
  // one wave per (layer, row j, slot s); blockIdx.x = (l * M + j) * t + s
  const int s = blockIdx.x % t;
  const int lj = blockIdx.x / t;
  const int j = lj % M, l = lj / M;
  const int p = parent[j];
  const size_t so = (size_t)l * layer_units + ((size_t)p * Lmax + s) * row_units + off_units;
  const size_t d0 = (size_t)l * layer_units + ((size_t)j * Lmax + s) * row_units + off_units;
  for (int64_t u = threadIdx.x; u < n_units; u += 64) dst[d0 + u] = src[so + u];
}

}  // namespace vct
using namespace vct;

template <int KMAX>
static void beam_launch(int dtype, int B, int K, int V, const void* x, int64_t ldx, bool vec_ok, float* pmax, float* psum,
                        float* ptv, int* pti, int CH, float* scores, uint8_t* finished, int32_t* parent, int64_t* out,
                        int64_t out_stride, int64_t end_id, int pad_id, int32_t* finished_count, unsigned long long* at, int t,
                        hipStream_t st) {
  const int M = B * K;
  if (dtype == VCT_BF16)
    vct::launch((beam_partial_kernel<bf16_t>), dim3(CH, M), dim3(BEAM_THREADS), 0, st, V, K, (const bf16_t*)x, ldx, vec_ok,
                pmax, psum, ptv, pti);
  else
    vct::launch((beam_partial_kernel<float>), dim3(CH, M), dim3(BEAM_THREADS), 0, st, V, K, (const float*)x, ldx, vec_ok,
                pmax, psum, ptv, pti);
  vct::launch((beam_merge_kernel<KMAX>), dim3(B), dim3(BEAM_THREADS), 0, st, K, V, CH, (const float*)pmax, (const float*)psum,
              (const float*)ptv, (const int*)pti, scores, finished, parent, out, out_stride, end_id, pad_id, M, finished_count, at, t);
}

extern "C" int vct_beam_select(int dtype, int B, int K, int V, const void* x, int64_t ldx, float* scores, uint8_t* finished,
                               int32_t* parent, int64_t* out, int64_t out_stride, int64_t end_id, int64_t pad_id,
                               int32_t* finished_count, int64_t* all_finished_at, int32_t t, void* workspace,
                               int64_t workspace_bytes, void* stream) {
  if (!dt_ok(dtype) || !x || !scores || !finished || !parent || !out || !finished_count || !all_finished_at || !workspace)
    return VCT_E_ARG;
  if (K < 1 || K > 16 || B <= 0 || V <= 0 || K > V || ldx < V || out_stride <= 0 || t < 0) return VCT_E_SHAPE;
  if (pad_id < 0 || pad_id >= V) return VCT_E_ARG;
  if ((int64_t)B * K > 65535 || (int64_t)K * V >= (int64_t)SEL_NONE) return VCT_E_SHAPE;
  const size_t CH = (size_t)sel_chunks(dtype, V);
  const size_t MC = (size_t)B * K * CH;
  if ((size_t)workspace_bytes < MC * (2 + 2 * (size_t)K) * 4) return VCT_E_WORKSPACE;
  float* pmax = (float*)workspace;
  float* psum = pmax + MC;
  float* ptv = psum + MC;
  int* pti = (int*)(ptv + MC * K);
  const size_t es = dtype == VCT_BF16 ? 2 : 4;
  const bool vec_ok = (((uintptr_t)x) & 15) == 0 && (((size_t)ldx * es) & 15) == 0;
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* at = reinterpret_cast<unsigned long long*>(all_finished_at);
  if (K <= 4)
    beam_launch<4>(dtype, B, K, V, x, ldx, vec_ok, pmax, psum, ptv, pti, (int)CH, scores, finished, parent, out, out_stride, end_id,
                   (int)pad_id, finished_count, at, (int)t, st);
  else if (K <= 8)
    beam_launch<8>(dtype, B, K, V, x, ldx, vec_ok, pmax, psum, ptv, pti, (int)CH, scores, finished, parent, out, out_stride, end_id,
                   (int)pad_id, finished_count, at, (int)t, st);
  else
    beam_launch<16>(dtype, B, K, V, x, ldx, vec_ok, pmax, psum, ptv, pti, (int)CH, scores, finished, parent, out, out_stride, end_id,
                    (int)pad_id, finished_count, at, (int)t, st);
  VCT_CHECK_LAUNCH();
  return VCT_OK;
}

extern "C" int vct_beam_reorder(int dtype, int L, int M, int Lmax, int d, int t, const int32_t* parent, const void* src, void* dst,
                                int64_t layer_stride, void* stream) {
  if (!dt_ok(dtype) || !parent || !src || !dst) return VCT_E_ARG;
  if (L <= 0 || M <= 0 || Lmax <= 0 || d <= 0 || t < 1 || t > Lmax) return VCT_E_SHAPE;
  if (layer_stride < (int64_t)M * Lmax * 3 * d) return VCT_E_SHAPE;
  if ((int64_t)L * M * t > 0x7fffffffLL) return VCT_E_SHAPE;
  if (src == dst) return VCT_E_ARG;              // no in-place gather: rows read and written by different waves
  hipStream_t st = (hipStream_t)stream;
  const size_t es = dtype == VCT_BF16 ? 2 : 4;
  const size_t row_b = 3 * (size_t)d * es, off_b = (size_t)d * es, n_b = 2 * (size_t)d * es, lay_b = (size_t)layer_stride * es;
  const dim3 grid((unsigned)((int64_t)L * M * t));
  const bool v16 = ((row_b | off_b | lay_b) & 15) == 0 && ((((uintptr_t)src) | ((uintptr_t)dst)) & 15) == 0;
  if (v16)
    vct::launch((beam_reorder_kernel<uint4>), grid, dim3(64), 0, st, M, Lmax, t, (int64_t)(row_b / 16), (int64_t)(off_b / 16),
                (int64_t)(n_b / 16), (int64_t)(lay_b / 16), parent, (const uint4*)src, (uint4*)dst);
  else if (es == 4)
    vct::launch((beam_reorder_kernel<uint32_t>), grid, dim3(64), 0, st, M, Lmax, t, (int64_t)(row_b / 4), (int64_t)(off_b / 4),
                (int64_t)(n_b / 4), (int64_t)(lay_b / 4), parent, (const uint32_t*)src, (uint32_t*)dst);
  else
    vct::launch((beam_reorder_kernel<uint16_t>), grid, dim3(64), 0, st, M, Lmax, t, (int64_t)(row_b / 2), (int64_t)(off_b / 2),
                (int64_t)(n_b / 2), (int64_t)(lay_b / 2), parent, (const uint16_t*)src, (uint16_t*)dst);
  VCT_CHECK_LAUNCH();
  return VCT_OK;
}
