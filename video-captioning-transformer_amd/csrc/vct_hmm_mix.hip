// Row routing between the layers of the hierarchical multi-modal encoder on gfx950 (include/vct_hip.h, vct_hmm_mix_*).
//
// replaces: the `inputs.append(last_output if target_layer[j] < i else ori_input[j])` + torch.cat of the reference's
// HMMEncoder.forward (model/MMEncoder.py:385-398) and its autograd backward (the split / cat backward and the sum of the
// stack input's gradient over the layers that restart from it).
//
// take uint8 [S], built by the host per layer: 1 = the row continues from the previous layer's output, 0 = it restarts from the
// stack input.
//   fwd, one launch:  x[b, s, :] = take[s] ? y[b, s, :] : x0[b, s, :]               (bitwise copy)
//   bwd, one launch, from the gradient dx of a layer's input:
//        dy[b, s, :]  = take[s] ? dx[b, s, :] : 0                                    (exact zeros)
//        acc[b, s, :] = take[s] ? 0 : float(dx)   with init;   += float(dx) on the restarting rows without it (others untouched)
//        with dx0 (layer 0: every row restarts):  dx0 = round(acc + float(dx)); neither dy nor acc is written, take is not read.
// One thread per 16-byte vector of a row; a thread owns its elements of acc from the first layer to the last, so the sum runs in
// layer order without atomics: bitwise reproducible.
#include "vct_common.h"

namespace vct {

constexpr int HM_THREADS = 256;
constexpr int HM_MAX_ROWS = 1024;

template <typename T, int VEC> struct alignas(sizeof(T) * VEC) HPack { T v[VEC]; };

template <typename T>
__global__ __launch_bounds__(HM_THREADS) void hmm_mix_fwd_kernel(const T* __restrict__ y, const T* __restrict__ x0, T* __restrict__ x,
                                                                 const uint8_t* __restrict__ take, int S, int nvec, long long total) {
  constexpr int VEC = 16 / sizeof(T);
  using P = HPack<T, VEC>;
  const long long it = (long long)blockIdx.x * HM_THREADS + threadIdx.x;
  if (it >= total) return;
  const long long row = it / nvec;
  const int s = (int)(row % S);
  const size_t at = (size_t)it * VEC;
  *reinterpret_cast<P*>(x + at) = *reinterpret_cast<const P*>((take[s] ? y : x0) + at);
}

template <typename T>
__global__ __launch_bounds__(HM_THREADS) void hmm_mix_bwd_kernel(const T* __restrict__ dx, T* __restrict__ dy, float* __restrict__ acc,
                                                                 T* __restrict__ dx0, const uint8_t* __restrict__ take, int init,
                                                                 int S, int nvec, long long total) {
  constexpr int VEC = 16 / sizeof(T);
  using P = HPack<T, VEC>;
  const long long it = (long long)blockIdx.x * HM_THREADS + threadIdx.x;
  if (it >= total) return;
  const size_t at = (size_t)it * VEC;
  const P g = *reinterpret_cast<const P*>(dx + at);
  float4* a4 = reinterpret_cast<float4*>(acc + at);
  if (dx0 != nullptr) {
    P o;
#pragma unroll
    for (int q = 0; q < VEC; q += 4) {
      const float4 a = a4[q / 4];
      o.v[q + 0] = from_f<T>(a.x + to_f<T>(g.v[q + 0]));
      o.v[q + 1] = from_f<T>(a.y + to_f<T>(g.v[q + 1]));
      o.v[q + 2] = from_f<T>(a.z + to_f<T>(g.v[q + 2]));
      o.v[q + 3] = from_f<T>(a.w + to_f<T>(g.v[q + 3]));
    }
    *reinterpret_cast<P*>(dx0 + at) = o;
    return;
  }
  const long long row = it / nvec;
  const bool t = take[(int)(row % S)] != 0;
  P o;
#pragma unroll
  for (int j = 0; j < VEC; j++) o.v[j] = t ? g.v[j] : (T)0;      // (the all-zero bit pattern is +0 in both formats)
  *reinterpret_cast<P*>(dy + at) = o;
  if (t && !init) return;
#pragma unroll
  for (int q = 0; q < VEC; q += 4) {
    float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (!t) {
      if (!init) a = a4[q / 4];
      a.x += to_f<T>(g.v[q + 0]); a.y += to_f<T>(g.v[q + 1]); a.z += to_f<T>(g.v[q + 2]); a.w += to_f<T>(g.v[q + 3]);
    }
    a4[q / 4] = a;
  }
}

}  // namespace vct
using namespace vct;

static bool hm_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }

// checks shared by both directions; nvec = 16-byte vectors per row, total = vectors in all B*S rows
static int hm_prepare(const vct_hmm_mix_desc* p, int& nvec, long long& total) {
  if (p == nullptr) return VCT_E_ARG;
  if (p->dtype != VCT_F32 && p->dtype != VCT_BF16) return VCT_E_ARG;
  if (p->B <= 0 || p->d <= 0 || p->S < 1 || p->S > HM_MAX_ROWS) return VCT_E_SHAPE;
  const int vec = p->dtype == VCT_BF16 ? 8 : 4;
  if (p->d % vec) return VCT_E_ALIGN;
  nvec = p->d / vec;
  total = (long long)p->B * p->S * nvec;
  if ((total + HM_THREADS - 1) / HM_THREADS > 0x7fffffffLL) return VCT_E_SHAPE;
  return VCT_OK;
}

extern "C" int vct_hmm_mix_fwd(const vct_hmm_mix_desc* p, void* stream) {
  int nvec; long long total;
  const int rc = hm_prepare(p, nvec, total);
  if (rc != VCT_OK) return rc;
  if (!p->take || !p->y || !p->x0 || !p->x) return VCT_E_ARG;
  if (!hm_aligned(p->y) || !hm_aligned(p->x0) || !hm_aligned(p->x)) return VCT_E_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)((total + HM_THREADS - 1) / HM_THREADS));
  if (p->dtype == VCT_BF16)
    vct::launch((hmm_mix_fwd_kernel<bf16_t>), grid, dim3(HM_THREADS), 0, st, (const bf16_t*)p->y, (const bf16_t*)p->x0, (bf16_t*)p->x,
                p->take, p->S, nvec, total);
  else
    vct::launch((hmm_mix_fwd_kernel<float>), grid, dim3(HM_THREADS), 0, st, (const float*)p->y, (const float*)p->x0, (float*)p->x,
                p->take, p->S, nvec, total);
  VCT_CHECK_LAUNCH();
  return VCT_OK;
}

extern "C" int vct_hmm_mix_bwd(const vct_hmm_mix_desc* p, void* stream) {
  int nvec; long long total;
  const int rc = hm_prepare(p, nvec, total);
  if (rc != VCT_OK) return rc;
  if (!p->dx || !p->acc) return VCT_E_ARG;
  if (p->dx0 != nullptr) {
    if (p->init) return VCT_E_ARG;            // the closing form reads an accumulator that an earlier launch initialised
  } else if (!p->take || !p->dy) {
    return VCT_E_ARG;
  }
  if (!hm_aligned(p->dx) || !hm_aligned(p->acc) || !hm_aligned(p->dy) || !hm_aligned(p->dx0)) return VCT_E_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)((total + HM_THREADS - 1) / HM_THREADS));
  const int init = p->init != 0;
  if (p->dtype == VCT_BF16)
    vct::launch((hmm_mix_bwd_kernel<bf16_t>), grid, dim3(HM_THREADS), 0, st, (const bf16_t*)p->dx, (bf16_t*)p->dy, p->acc, (bf16_t*)p->dx0,
                p->take, init, p->S, nvec, total);
  else
    vct::launch((hmm_mix_bwd_kernel<float>), grid, dim3(HM_THREADS), 0, st, (const float*)p->dx, (float*)p->dy, p->acc, (float*)p->dx0,
                p->take, init, p->S, nvec, total);
  VCT_CHECK_LAUNCH();
  return VCT_OK;
}
