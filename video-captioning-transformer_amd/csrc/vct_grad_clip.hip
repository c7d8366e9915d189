// Gradient clipping over the flat fp32 gradient buffer: the global L2 norm (and the norm of every parameter) in two launches, the
// scaling or the value clamp in one.  replaces torch.nn.utils.clip_grad_norm_ / clip_grad_value_ (some seventy per-tensor norms, a
// stack, a norm of norms, a clamp and a foreach multiply on the host route).
//
// The buffer is described by a device table of SEGMENTS (one per parameter: the alignment padding between parameters is never
// read or written).  The workgroup -> elements map is vct_adam_step_ranges': GRAD_EPB elements per workgroup, blk0 = workgroups of all
// earlier segments, binary search on blk0.  A segment begins at a multiple of 4 (16-byte vectors) and ends anywhere: the last
// vector of a segment that is not whole is handled element by element, so nothing behind `end` is touched.
//
// Determinism: no atomics anywhere.  Pass 1 leaves ONE fp64 partial per workgroup (per-thread sums in element order, a fixed
// shuffle tree over the wave, the four wave sums added in wave order); pass 2 adds the partials of a segment with a fixed lane
// stride and the same tree, and the segment sums in ascending segment order.  Two runs give the same bits.
// fp64: a square of 3e19 overflows fp32 and one of 1e-30 vanishes in it; the product of two fp32 values is exact in fp64, and an
// fp64 sum over 5e7 terms is good to ~1e-9 relative, so the fp32 norm that comes out is the correctly rounded one but for the last
// bit.  HBM-bound all the same: 4 B read per element against one conversion and one fp64 FMA.
#include "vct_common.h"

namespace vct {

struct GradSeg { int64_t begin, end; int32_t blk0, reserved; };
constexpr int GRAD_EPB = 4096;

// the segment of this workgroup and its elements [e0, e1)
__device__ __forceinline__ void grad_block_range(const GradSeg* __restrict__ segs, int nseg, int64_t& e0, int64_t& e1) {
  int lo = 0, hi = nseg;                                     // last segment whose first workgroup is <= this one
  while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (segs[mid].blk0 <= (int)blockIdx.x) lo = mid; else hi = mid; }
  const GradSeg sg = segs[lo];
  e0 = sg.begin + (int64_t)((int)blockIdx.x - sg.blk0) * GRAD_EPB;
  e1 = e0 + GRAD_EPB < sg.end ? e0 + GRAD_EPB : sg.end;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// ---- pass 1: one fp64 partial sum of squares per workgroup ----------------------------------------------------------------------
__global__ __launch_bounds__(256) void grad_sqnorm_partial_kernel(const float* __restrict__ g, const GradSeg* __restrict__ segs, int nseg,
                                                                  double* __restrict__ partials) {
  __shared__ double red[4];
  int64_t e0, e1;
  grad_block_range(segs, nseg, e0, e1);
  float4 v[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {                              // the (up to) four 16-byte loads of the thread first
    const int64_t e = e0 + (int64_t)threadIdx.x * 4 + (int64_t)k * 1024;
    v[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (e + 4 <= e1) {
      v[k] = *reinterpret_cast<const float4*>(g + e);
    } else if (e < e1) {                                     // the tail of the segment: element by element, nothing behind `end`
      float* vp = &v[k].x;
      for (int j = 0; j < 4; j++) if (e + j < e1) vp[j] = g[e + j];
    }
  }
  double acc = 0.0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const float* vp = &v[k].x;
#pragma unroll
    for (int j = 0; j < 4; j++) { const double x = (double)vp[j]; acc = fma(x, x, acc); }
  }
  acc = wave_sum_f64(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// ---- pass 2: one workgroup; a wave per segment, then the segments in ascending order ------------------------------------------------
// seg_sums: fp64 [nseg] scratch behind the partials.  state = {norm, coef, 0, 0}.
constexpr int GRAD_FIN_WAVES = 16;
__global__ __launch_bounds__(GRAD_FIN_WAVES * 64) void grad_sqnorm_finish_kernel(const GradSeg* __restrict__ segs, int nseg, int total_blocks,
                                                                               const double* __restrict__ partials,
                                                                               double* __restrict__ seg_sums, float* __restrict__ seg_norm,
                                                                               const float* __restrict__ clip, float* __restrict__ state) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int s = wave; s < nseg; s += GRAD_FIN_WAVES) {
    const int b0 = segs[s].blk0;
    const int b1 = s + 1 < nseg ? segs[s + 1].blk0 : total_blocks;
    double acc = 0.0;
    for (int b = b0 + lane; b < b1; b += 64 * 16) {          // lane l adds partials l, l + 64, ... in ascending order, 16 loads in flight
      double p[16];
#pragma unroll
      for (int u = 0; u < 16; u++) p[u] = b + 64 * u < b1 ? partials[b + 64 * u] : 0.0;   // (+0.0 leaves a sum of squares as it is)
#pragma unroll
      for (int u = 0; u < 16; u++) acc += p[u];
    }
    acc = wave_sum_f64(acc);
    if (lane == 0) {
      seg_sums[s] = acc;
      seg_norm[s] = (float)sqrt(acc);
    }
  }
  __syncthreads();                                           // the segment sums of every wave are visible to wave 0
  if (wave != 0) return;
  double tot = 0.0;
  for (int s0 = 0; s0 < nseg; s0 += 64) {                    // 64 sums per load, added one by one in ascending segment order
    const double mine = s0 + lane < nseg ? seg_sums[s0 + lane] : 0.0;
#pragma unroll
    for (int j = 0; j < 64; j++) tot += __shfl(mine, j);
  }
  if (lane == 0) {
    const float norm = (float)sqrt(tot);
    const float q = clip[0] / (norm + 1e-6f);
    state[0] = norm;
    state[1] = q > 1.0f ? 1.0f : q;                          // a NaN stays (torch.clamp(max = 1.0))
    state[2] = 0.0f;
    state[3] = 0.0f;
  }
}

// ---- apply: g *= coef (mode 0) or g = clamp(g, -v, v) (mode 1) ---------------------------------------------------------------------
__device__ __forceinline__ float clamp_like_torch(float x, float v) { return x < -v ? -v : (x > v ? v : x); }   // NaN and -0.0 pass

template <int MODE>
__global__ __launch_bounds__(256) void grad_clip_apply_kernel(float* __restrict__ g, const GradSeg* __restrict__ segs, int nseg,
                                                              const float* __restrict__ clip, const float* __restrict__ state) {
  const float c = MODE == 0 ? state[1] : clip[1];
  if (MODE == 0 && c == 1.0f) return;                        // bitwise the multiplication by one: nothing is read or written
  int64_t e0, e1;
  grad_block_range(segs, nseg, e0, e1);
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int64_t e = e0 + (int64_t)threadIdx.x * 4 + (int64_t)k * 1024;
    if (e + 4 <= e1) {
      float4 v = *reinterpret_cast<const float4*>(g + e);
      float* vp = &v.x;
#pragma unroll
      for (int j = 0; j < 4; j++) vp[j] = MODE == 0 ? vp[j] * c : clamp_like_torch(vp[j], c);
      *reinterpret_cast<float4*>(g + e) = v;
    } else if (e < e1) {
      for (int j = 0; j < 4; j++) if (e + j < e1) g[e + j] = MODE == 0 ? g[e + j] * c : clamp_like_torch(g[e + j], c);
    }
  }
}

}  // namespace vct
using namespace vct;

extern "C" int vct_grad_sqnorm(const float* grad, const vct_grad_seg* segs_dev, int32_t nseg, int32_t total_blocks, double* partials,
                               float* seg_norm, const float* clip_dev, float* state, void* stream) {
  static_assert(sizeof(vct_grad_seg) == sizeof(GradSeg), "descriptor layout");
  if (!grad || !segs_dev || !partials || !seg_norm || !clip_dev || !state) return VCT_E_ARG;
  if (nseg <= 0 || total_blocks <= 0) return VCT_E_SHAPE;
  if (((uintptr_t)grad | (uintptr_t)partials | (uintptr_t)segs_dev) & 15) return VCT_E_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  const GradSeg* segs = reinterpret_cast<const GradSeg*>(segs_dev);
  vct::launch(grad_sqnorm_partial_kernel, dim3(total_blocks), dim3(256), 0, st, grad, segs, (int)nseg, partials);
  VCT_CHECK_LAUNCH();
  vct::launch(grad_sqnorm_finish_kernel, dim3(1), dim3(GRAD_FIN_WAVES * 64), 0, st, segs, (int)nseg, (int)total_blocks,
              (const double*)partials, partials + total_blocks, seg_norm, clip_dev, state);
  VCT_CHECK_LAUNCH();
  return VCT_OK;
}

extern "C" int vct_grad_clip_apply(float* grad, const vct_grad_seg* segs_dev, int32_t nseg, int32_t total_blocks, int32_t mode,
                                   const float* clip_dev, const float* state, void* stream) {
  if (!grad || !segs_dev || !clip_dev || (mode == 0 && !state)) return VCT_E_ARG;
  if (mode != 0 && mode != 1) return VCT_E_ARG;
  if (nseg <= 0 || total_blocks <= 0) return VCT_E_SHAPE;
  if (((uintptr_t)grad | (uintptr_t)segs_dev) & 15) return VCT_E_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  const GradSeg* segs = reinterpret_cast<const GradSeg*>(segs_dev);
  if (mode == 0)
    vct::launch(grad_clip_apply_kernel<0>, dim3(total_blocks), dim3(256), 0, st, grad, segs, (int)nseg, clip_dev, state);
  else
    vct::launch(grad_clip_apply_kernel<1>, dim3(total_blocks), dim3(256), 0, st, grad, segs, (int)nseg, clip_dev, state);
  VCT_CHECK_LAUNCH();
  return VCT_OK;
}
