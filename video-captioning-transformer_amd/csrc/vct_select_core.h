// Shared device code of the token-selection kernels: greedy (vct_select.hip, the tail of decode_gen_kernel in
// vct_decode_block.hip), beam (vct_beam.hip) and sampled (vct_sample.hip).  One definition each of
//   the tie rule     larger value wins, equal values go to the smaller index (torch.max's first-index rule); SEL_NONE is the
//                    empty entry that loses to everything, -inf valued real candidates included.  A NaN never wins.
//   the chunk scan   256 threads x one 16-byte load of a row -> the thread's head, the chunk's max, its sum of exponentials and
//                    its top K by K rounds of a workgroup arg-max (shuffles, then one LDS exchange per round)
//   the end of sequence bookkeeping   sticky flag, integer count, step at which the count reached the total.
// Reductions have a fixed order (shuffle tree, then the waves in order): no floating-point atomics.
#pragma once
#include "vct_common.h"

namespace vct {

constexpr int SEL_NONE = 0x7fffffff;
constexpr int SEL_THREADS = 256;            // the chunk geometry: a chunk is SEL_THREADS x 16 bytes of a row
constexpr int SEL_WAVES = SEL_THREADS / 64;

__device__ __forceinline__ bool sel_better(float av, int ai, float bv, int bi) { return av > bv || (av == bv && ai < bi); }

// (value, index) arg-max over the 64 lanes of a wave
__device__ __forceinline__ void sel_wave_best(float& v, int& i) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o);
    const int oi = __shfl_xor(i, o);
    if (sel_better(ov, oi, v, i)) { v = ov; i = oi; }
  }
}

// the best of the NW waves' pairs in LDS (s_v[w], s_i[w]: what lane 0 of wave w stored after sel_wave_best)
template <int NW>
__device__ __forceinline__ void sel_fold_waves(float& v, int& i, const float* s_v, const int* s_i) {
  v = s_v[0]; i = s_i[0];
#pragma unroll
  for (int u = 1; u < NW; u++)
    if (sel_better(s_v[u], s_i[u], v, i)) { v = s_v[u]; i = s_i[u]; }
}

// workgroup (NW waves) arg-max of every thread's (v, i), to every thread.  The LDS pair is double-buffered by round parity, so one
// barrier per round.
template <int NW>
__device__ __forceinline__ void sel_block_best(float& v, int& i, float (*s_v)[NW], int (*s_i)[NW], int round) {
  sel_wave_best(v, i);
  const int w = threadIdx.x >> 6, p = round & 1;
  if ((threadIdx.x & 63) == 0) { s_v[p][w] = v; s_i[p][w] = i; }
  __syncthreads();
  sel_fold_waves<NW>(v, i, s_v[p], s_i[p]);
}

// the thread's VEC = 16 / sizeof(T) elements of a chunk, from column c0: values (fp32) and columns; -inf / SEL_NONE past V
template <typename T, int VEC>
__device__ __forceinline__ void sel_chunk_load(const T* __restrict__ r, int c0, int V, bool vec_ok, float (&e)[VEC], int (&id)[VEC]) {
  if (vec_ok && c0 + VEC <= V) {
    struct alignas(16) Vt { T e[VEC]; };
    const Vt w = *reinterpret_cast<const Vt*>(r + c0);
#pragma unroll
    for (int u = 0; u < VEC; u++) { e[u] = to_f<T>(w.e[u]); id[u] = c0 + u; }
  } else {
#pragma unroll
    for (int u = 0; u < VEC; u++) {
      const bool in = c0 + u < V;
      e[u] = in ? to_f<T>(r[c0 + u]) : -INFINITY;
      id[u] = in ? c0 + u : SEL_NONE;
    }
  }
}

// the thread's head: the best of its remaining elements
template <int VEC>
__device__ __forceinline__ void sel_head(const float (&e)[VEC], const int (&id)[VEC], float& hv, int& hi) {
  hv = -INFINITY; hi = SEL_NONE;
#pragma unroll
  for (int u = 0; u < VEC; u++)
    if (sel_better(e[u], id[u], hv, hi)) { hv = e[u]; hi = id[u]; }
}

// the chunk's sum of exp(x * inv_temp - zm), in thread 0 (s_sum: SEL_WAVES floats)
template <int VEC>
__device__ __forceinline__ float sel_chunk_expsum(const float (&e)[VEC], const int (&id)[VEC], float inv_temp, float zm, float* s_sum) {
  float se = 0.0f;
#pragma unroll
  for (int u = 0; u < VEC; u++) se += (id[u] != SEL_NONE) ? expf(e[u] * inv_temp - zm) : 0.0f;
  se = wave_sum(se);
  if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = se;
  __syncthreads();
  float t = 0.0f;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 0; w < SEL_WAVES; w++) t += s_sum[w];
  }
  return t;
}

// the chunk's top K (value, column) in rank order -> ptv / pti [pc * stride + k].  Round 0's winner is the chunk's max (mv, mi),
// found before; after each round the owner drops its element and finds its next head (hv, hi).
template <int VEC>
__device__ __forceinline__ void sel_chunk_topk(int K, float (&e)[VEC], int (&id)[VEC], float& hv, int& hi, float mv, int mi,
                                               float (*s_v)[SEL_WAVES], int (*s_i)[SEL_WAVES], float* __restrict__ ptv,
                                               int* __restrict__ pti, size_t pc, int stride) {
  for (int k = 0; k < K; k++) {
    float bv = hv;
    int bi = hi;
    if (k > 0) sel_block_best<SEL_WAVES>(bv, bi, s_v, s_i, k);
    else { bv = mv; bi = mi; }
    if (threadIdx.x == 0) { ptv[pc * stride + k] = bv; pti[pc * stride + k] = bi; }
    if (bi == hi && bi != SEL_NONE) {
#pragma unroll
      for (int u = 0; u < VEC; u++)
        if (id[u] == bi) { id[u] = SEL_NONE; e[u] = -INFINITY; }
      sel_head(e, id, hv, hi);
    }
  }
}

// End-of-sequence bookkeeping (MMT4Caption.py:166-171), by one thread: n rows end with step t.  The row's flag is sticky (the
// caller tests it first; beam search keeps its flags per slot and passes nullptr); the arrival that completes the set of `total`
// records the step.  Integer atomics only: the result does not depend on arrival order.
__device__ __forceinline__ void sel_mark_ended(uint8_t* flag, int n, int32_t* count, int total, unsigned long long* at, int t) {
  if (flag != nullptr) *flag = 1;
  if (n > 0 && atomicAdd(count, n) + n == total) atomicMin(at, (unsigned long long)t);
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
static inline bool dt_ok(int dt) { return dt == VCT_F32 || dt == VCT_BF16; }

// chunks of a V-column row
static inline int64_t sel_chunks(int dtype, int V) {
  const int chunk = SEL_THREADS * (dtype == VCT_BF16 ? 8 : 4);
  return ((int64_t)V + chunk - 1) / chunk;
}

}  // namespace vct
