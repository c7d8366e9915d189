// Greedy token selection on gfx950: the row arg-max (torch.max's first-index rule) and, for the decode loop, its end-of-sequence
// bookkeeping in the same launch.
//
// replaces: the reference's greedy step (MMT4Caption.py:166-171: torch.max over the vocabulary, then the per-row end flags).
//
// One workgroup of 1024 threads per row: 16-byte loads over the whole row where it allows them, a scalar tail, then one workgroup
// arg-max.  The tie rule, the reductions and the bookkeeping are vct_select_core.h's, shared with vct_beam.hip and vct_sample.hip.
#include "vct_select_core.h"

namespace vct {

constexpr int AMX_THREADS = 1024;
template <typename T>
__global__ __launch_bounds__(AMX_THREADS) void argmax_rows_kernel(int cols, const T* __restrict__ x, int64_t ldx,
                                                                  int64_t* __restrict__ out, int64_t out_stride, int64_t end_id,
                                                                  uint8_t* __restrict__ ended, int32_t* __restrict__ ended_count,
                                                                  unsigned long long* __restrict__ all_ended_at, int t) {
  __shared__ float s_v[AMX_THREADS / 64];
  __shared__ int s_i[AMX_THREADS / 64];
  const T* r = x + (size_t)blockIdx.x * ldx;
  float best = -INFINITY;
  int bi = SEL_NONE;
  // 16-byte loads when the row allows it (a 30522-column row is 4 vector loads per thread instead of 30 scalar round trips:
  // the one-workgroup-per-row scan took 37 us per decoded token)
  constexpr int VEC = 16 / (int)sizeof(T);
  const bool vec_ok = (((uintptr_t)r) & 15) == 0;
  const int nv = vec_ok ? cols / VEC : 0;
  struct alignas(16) V { T e[VEC]; };
  for (int j = threadIdx.x; j < nv; j += AMX_THREADS) {
    const V v = reinterpret_cast<const V*>(r)[j];
#pragma unroll
    for (int u = 0; u < VEC; u++) {
      const float f = to_f<T>(v.e[u]);
      if (sel_better(f, j * VEC + u, best, bi)) { best = f; bi = j * VEC + u; }
    }
  }
  for (int j = nv * VEC + threadIdx.x; j < cols; j += AMX_THREADS) {
    const float v = to_f<T>(r[j]);
    if (sel_better(v, j, best, bi)) { best = v; bi = j; }
  }
  sel_wave_best(best, bi);
  if ((threadIdx.x & 63) == 0) { s_v[threadIdx.x >> 6] = best; s_i[threadIdx.x >> 6] = bi; }
  __syncthreads();
  if (threadIdx.x == 0) {                   // one row, one result: thread 0 alone folds the 16 waves
    sel_fold_waves<AMX_THREADS / 64>(best, bi, s_v, s_i);
    const int tok = (bi == SEL_NONE) ? 0 : bi;
    out[(size_t)blockIdx.x * out_stride] = tok;
    if (ended != nullptr && tok == end_id && !ended[blockIdx.x])
      sel_mark_ended(&ended[blockIdx.x], 1, ended_count, (int)gridDim.x, all_ended_at, t);
  }
}

}  // namespace vct
using namespace vct;

// ended == nullptr: the arg-max alone
static int argmax_launch(int dtype, int rows, int cols, const void* x, int64_t ldx, int64_t* out, int64_t out_stride, int64_t end_id,
                         uint8_t* ended, int32_t* ended_count, int64_t* all_ended_at, int t, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* at = reinterpret_cast<unsigned long long*>(all_ended_at);
  if (dtype == VCT_BF16)
    vct::launch((argmax_rows_kernel<bf16_t>), dim3(rows), dim3(AMX_THREADS), 0, st, cols, (const bf16_t*)x, ldx, out, out_stride,
                end_id, ended, ended_count, at, t);
  else
    vct::launch((argmax_rows_kernel<float>), dim3(rows), dim3(AMX_THREADS), 0, st, cols, (const float*)x, ldx, out, out_stride,
                end_id, ended, ended_count, at, t);
  VCT_CHECK_LAUNCH();
  return VCT_OK;
}

extern "C" int vct_argmax_rows(int dtype, int rows, int cols, const void* x, int64_t ldx, int64_t* out, int64_t out_stride,
                               void* stream) {
  if (!dt_ok(dtype) || !x || !out) return VCT_E_ARG;
  if (rows <= 0 || cols <= 0 || out_stride <= 0) return VCT_E_SHAPE;
  return argmax_launch(dtype, rows, cols, x, ldx, out, out_stride, 0, nullptr, nullptr, nullptr, 0, stream);
}

extern "C" int vct_greedy_select(int dtype, int rows, int cols, const void* x, int64_t ldx, int64_t* out, int64_t out_stride,
                                 int64_t end_id, uint8_t* ended, int32_t* ended_count, int64_t* all_ended_at, int32_t t,
                                 void* stream) {
  if (!dt_ok(dtype) || !x || !out || !ended || !ended_count || !all_ended_at) return VCT_E_ARG;
  if (rows <= 0 || cols <= 0 || out_stride <= 0 || t < 0) return VCT_E_SHAPE;
  return argmax_launch(dtype, rows, cols, x, ldx, out, out_stride, end_id, ended, ended_count, all_ended_at, (int)t, stream);
}
