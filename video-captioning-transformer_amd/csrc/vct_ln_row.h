// One wave normalises one fp32 row held in registers: the LayerNorm of the frozen CLIP towers (vct_text.hip, vct_vision.hip).
// float4 loads, <= 16 values per lane => d <= 1024 (a multiple of 4), two-pass variance in fp32 -- the scheme of vct_norm.hip.
#pragma once
#include "vct_common.h"

namespace vct {

constexpr int TXT_MAXIT = 4;   // 4 x 64 lanes x float4 = 1024 columns

template <typename T> struct alignas(sizeof(T) * 4) Out4 { T v[4]; };

// the row is in `s` (lane's vectors it * 64 + lane, zeros behind d), `sum` is the lane's sum of it; every lane of the wave takes part
template <typename T>
__device__ __forceinline__ void ln_regs(float (&s)[TXT_MAXIT][4], float sum, const float* __restrict__ gamma,
                                        const float* __restrict__ beta, T* __restrict__ dst, int d, int lane) {
  const int nvec = d >> 2;
  const float mean = wave_sum(sum) / (float)d;
  float sq = 0.0f;
#pragma unroll
  for (int it = 0; it < TXT_MAXIT; it++) {
    if (it * 64 + lane < nvec) {
#pragma unroll
      for (int j = 0; j < 4; j++) { const float c = s[it][j] - mean; sq += c * c; }
    }
  }
  const float rstd = 1.0f / sqrtf(wave_sum(sq) / (float)d + 1e-5f);
#pragma unroll
  for (int it = 0; it < TXT_MAXIT; it++) {
    const int vi = it * 64 + lane;
    if (vi < nvec) {
      const float4 g = *reinterpret_cast<const float4*>(gamma + vi * 4);
      const float4 b = *reinterpret_cast<const float4*>(beta + vi * 4);
      Out4<T> o;
      o.v[0] = from_f<T>((s[it][0] - mean) * rstd * g.x + b.x);
      o.v[1] = from_f<T>((s[it][1] - mean) * rstd * g.y + b.y);
      o.v[2] = from_f<T>((s[it][2] - mean) * rstd * g.z + b.z);
      o.v[3] = from_f<T>((s[it][3] - mean) * rstd * g.w + b.w);
      *reinterpret_cast<Out4<T>*>(dst + vi * 4) = o;
    }
  }
}

// normalises the row `src` (d columns, fp32) into `dst`; every lane of the wave takes part
template <typename T>
__device__ __forceinline__ void ln_row(const float* __restrict__ src, const float* __restrict__ gamma, const float* __restrict__ beta,
                                       T* __restrict__ dst, int d, int lane) {
  const int nvec = d >> 2;
  float s[TXT_MAXIT][4];
  float sum = 0.0f;
#pragma unroll
  for (int it = 0; it < TXT_MAXIT; it++) {
    const int vi = it * 64 + lane;
    if (vi < nvec) {
      const float4 v = *reinterpret_cast<const float4*>(src + vi * 4);
      s[it][0] = v.x; s[it][1] = v.y; s[it][2] = v.z; s[it][3] = v.w;
      sum += (v.x + v.y) + (v.z + v.w);
    } else {
#pragma unroll
      for (int j = 0; j < 4; j++) s[it][j] = 0.0f;
    }
  }
  ln_regs<T>(s, sum, gamma, beta, dst, d, lane);
}

// the shape rules both towers' LayerNorm entry points share
static inline int ln_row_check(int out_dtype, int d) {
  if (out_dtype != VCT_F32 && out_dtype != VCT_BF16) return VCT_E_ARG;
  if (d <= 0) return VCT_E_SHAPE;
  if (d % 4) return VCT_E_ALIGN;
  if (d > 1024) return VCT_E_SHAPE;
  return VCT_OK;
}

}  // namespace vct
