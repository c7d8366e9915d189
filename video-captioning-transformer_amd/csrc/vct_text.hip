// The two kernels of the frozen CLIP text tower that the rest of the library cannot express (text.py).  Everything else of
// the tower is vct_embed_fwd, vct_gemm and vct_attn_fwd.
//   vct_preln_fwd : y = LayerNorm(x), x the FP32 residual stream, y in the compute dtype.  A pre-LN stack adds a small update to the
//                   stream in every layer, so the stream stays fp32 while the GEMM operands are bf16; vct_add_ln_fwd takes one dtype
//                   for both sides and saves statistics that a forward-only tower never reads.
//   vct_text_pool : per caption the FIRST index of the largest id (CLIP's `text.argmax(dim=-1)`: the EOT token has the largest id),
//                   that row of the stream through ln_final, in the compute dtype.
// Both: one wave per row, the row in registers (float4 loads, <= 16 values per lane => d <= 1024), two-pass variance in fp32 -- the
// scheme of vct_norm.hip (vct_ln_row.h, shared with the vision tower).  HBM-bound; nothing is staged in LDS.
#include "vct_common.h"
#include "vct_ln_row.h"

namespace vct {

template <typename T>
__global__ __launch_bounds__(256) void preln_fwd_kernel(int M, int d, const float* __restrict__ x, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, T* __restrict__ y) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;   // whole waves leave: no shuffle below runs with missing lanes
  ln_row<T>(x + (size_t)row * d, gamma, beta, y + (size_t)row * d, d, lane);
}

// ids: [B, ld_ids] int64, the first Lids columns of a row are scanned; x: [B * L, d].  A caption whose first maximum lies at or
// behind L (the host trimmed too far) raises *err and gets a zero row: its stream row does not exist.
template <typename T>
__global__ __launch_bounds__(256) void text_pool_kernel(int B, int L, int Lids, int d, const int64_t* __restrict__ ids, int64_t ld_ids,
                                                        const float* __restrict__ x, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, T* __restrict__ y, int32_t* __restrict__ eot,
                                                        int32_t* __restrict__ err) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const int64_t* row = ids + (size_t)b * ld_ids;
  long long best = INT64_MIN;
  int at = 0x7fffffff;
  for (int l = lane; l < Lids; l += 64) {
    const long long v = row[l];
    if (at == 0x7fffffff || v > best) { best = v; at = l; }   // strictly greater: a lane keeps its first maximum
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const long long ob = __shfl_xor(best, o);
    const int oa = __shfl_xor(at, o);
    // lanes without a column (Lids < 64) carry at = INT_MAX and lose against every real column
    const bool take = (oa != 0x7fffffff) && (at == 0x7fffffff || ob > best || (ob == best && oa < at));
    if (take) { best = ob; at = oa; }
  }
  if (lane == 0) eot[b] = at;
  T* dst = y + (size_t)b * d;
  if (at >= L) {
    if (lane == 0) *err = 1;
    for (int c = lane * 4; c < d; c += 256) {
      Out4<T> z;
#pragma unroll
      for (int j = 0; j < 4; j++) z.v[j] = from_f<T>(0.0f);
      *reinterpret_cast<Out4<T>*>(dst + c) = z;
    }
    return;   // wave-uniform: `at` is the same in every lane after the butterfly
  }
  ln_row<T>(x + ((size_t)b * L + at) * d, gamma, beta, dst, d, lane);
}

}  // namespace vct

using namespace vct;

extern "C" int vct_preln_fwd(int out_dtype, int M, int d, const float* x, const float* gamma, const float* beta, void* y, void* stream) {
  if (!x || !gamma || !beta || !y) return VCT_E_ARG;
  const int rc = ln_row_check(out_dtype, d);
  if (rc) return rc;
  if (M <= 0) return VCT_E_SHAPE;
  if (((uintptr_t)x | (uintptr_t)gamma | (uintptr_t)beta) & 15) return VCT_E_ALIGN;
  if ((uintptr_t)y & (out_dtype == VCT_BF16 ? 7 : 15)) return VCT_E_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  if (out_dtype == VCT_BF16)
    vct::launch((preln_fwd_kernel<bf16_t>), dim3((M + 3) / 4), dim3(256), 0, st, M, d, x, gamma, beta, (bf16_t*)y);
  else
    vct::launch((preln_fwd_kernel<float>), dim3((M + 3) / 4), dim3(256), 0, st, M, d, x, gamma, beta, (float*)y);
  VCT_CHECK_LAUNCH();
  return VCT_OK;
}

extern "C" int vct_text_pool(int out_dtype, int B, int L, int Lids, int d, const int64_t* ids, int64_t ld_ids, const float* x,
                             const float* gamma, const float* beta, void* y, int32_t* eot, int32_t* err, void* stream) {
  if (!ids || !x || !gamma || !beta || !y || !eot || !err) return VCT_E_ARG;
  const int rc = ln_row_check(out_dtype, d);
  if (rc) return rc;
  if (B <= 0 || L <= 0 || Lids < L || ld_ids < Lids) return VCT_E_SHAPE;
  if (((uintptr_t)x | (uintptr_t)gamma | (uintptr_t)beta) & 15) return VCT_E_ALIGN;
  if (((uintptr_t)y & (out_dtype == VCT_BF16 ? 7 : 15)) || ((uintptr_t)ids & 7) || (((uintptr_t)eot | (uintptr_t)err) & 3)) return VCT_E_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  if (out_dtype == VCT_BF16)
    vct::launch((text_pool_kernel<bf16_t>), dim3((B + 3) / 4), dim3(256), 0, st, B, L, Lids, d, ids, ld_ids, x, gamma, beta, (bf16_t*)y,
                eot, err);
  else
    vct::launch((text_pool_kernel<float>), dim3((B + 3) / 4), dim3(256), 0, st, B, L, Lids, d, ids, ld_ids, x, gamma, beta, (float*)y,
                eot, err);
  VCT_CHECK_LAUNCH();
  return VCT_OK;
}
