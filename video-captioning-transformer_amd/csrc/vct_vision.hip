// The three kernels of the frozen CLIP vision tower that the rest of the library cannot express (vision.py).  The block
// itself is vct_preln_fwd, vct_gemm and vct_attn_fwd, as in the text tower.
//   vct_frames_to_patches : uint8 frames -> the patch-embedding GEMM's A operand: PIL's integer bicubic resize (shorter side to R),
//                           centre crop, ToTensor and Normalize.  The host owns every fp64 decision (the two coefficient tables) and
//                           every fp32 one (the [3][256] value table); the kernel does integer taps and a lookup, so each output is
//                           exact by construction.  One workgroup per (frame, patch): the horizontal pass of the input rows the patch
//                           needs goes to LDS as uint8, the vertical pass reads it there -- PIL's order, and its uint8 intermediate.
//   vct_vit_embed         : class token / patch rows + positions, then ln_pre, into the fp32 residual stream.
//   vct_vit_pool          : ln_post of the class rows, in the compute dtype.
// The LayerNorm kernels: one wave per row, the row in registers (vct_ln_row.h).  All three are HBM-bound.
#include "vct_common.h"
#include "vct_ln_row.h"

namespace vct {

constexpr int F2P_THREADS = 256;
constexpr int F2P_LDS_MAX = 65536;
constexpr int F2P_PB = 22;          // PIL's PRECISION_BITS for 8-bit channels

// LDS of one workgroup: wx [P * kx] | wy [P * ky] | xmin, xlen, ymin, ylen [P each] (int32) | stage [rows * P * 3] | res [P * P * 3] (uint8)
static inline long long f2p_lds_bytes(int P, int kx, int ky, int stage_rows) {
  const long long ints = (long long)P * kx + (long long)P * ky + 4LL * P;
  const long long stage = ((long long)stage_rows * P * 3 + 15) / 16 * 16;
  return ints * 4 + stage + (long long)P * P * 3;
}

__device__ __forceinline__ int clip8(int acc) {
  const int v = acc >> F2P_PB;      // arithmetic shift, as PIL's
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// frames [N, H, W, 3]; hx_*: the R cropped columns of the horizontal pass (window start in input columns, length, kx padded weights);
// vy_*: the R cropped rows of the vertical pass (window start in input rows).  A pass that PIL skips is a one-tap table of weight 2^22,
// which returns the byte unchanged.  out: row (n * G + gy) * G + gx, column c * P * P + py * P + px; crop (or NULL): [N, R, R, 3].
template <typename T>
__global__ __launch_bounds__(F2P_THREADS) void frames_to_patches_kernel(
    int H, int W, int R, int P, int G, const uint8_t* __restrict__ frames, const int32_t* __restrict__ hx_min,
    const int32_t* __restrict__ hx_len, const int32_t* __restrict__ hx_w, int kx, const int32_t* __restrict__ vy_min,
    const int32_t* __restrict__ vy_len, const int32_t* __restrict__ vy_w, int ky, int stage_rows, const T* __restrict__ lut,
    T* __restrict__ out, uint8_t* __restrict__ crop) {
  extern __shared__ __attribute__((aligned(16))) uint8_t f2p_smem[];
  int32_t* wx = reinterpret_cast<int32_t*>(f2p_smem);
  int32_t* wy = wx + P * kx;
  int32_t* xmin = wy + P * ky;
  int32_t* xlen = xmin + P;
  int32_t* ymin = xlen + P;
  int32_t* ylen = ymin + P;
  uint8_t* stage = reinterpret_cast<uint8_t*>(ylen + P);
  uint8_t* res = stage + ((size_t)stage_rows * P * 3 + 15) / 16 * 16;

  const int tid = threadIdx.x;
  const int patch = blockIdx.x;
  const int gx = patch % G, gy = (patch / G) % G;
  const int n = patch / (G * G);
  const int c0 = gx * P, r0 = gy * P;

  // the tables of this patch's P columns and P rows.  Windows are clamped to the frame and to the staged rows: a table that is
  // not the host's own cannot make a load or an LDS access leave its array
  for (int i = tid; i < P * kx; i += F2P_THREADS) wx[i] = hx_w[(size_t)c0 * kx + i];
  for (int i = tid; i < P * ky; i += F2P_THREADS) wy[i] = vy_w[(size_t)r0 * ky + i];
  const int lo = min(max(vy_min[r0], 0), H - 1);
  const int last = min(max(vy_min[r0 + P - 1], lo), H - 1);
  const int nrows = min(min(last + max(min(vy_len[r0 + P - 1], ky), 0), H) - lo, stage_rows);
  for (int i = tid; i < P; i += F2P_THREADS) {
    const int x0 = min(max(hx_min[c0 + i], 0), W - 1);
    xmin[i] = x0;
    xlen[i] = max(min(min(hx_len[c0 + i], kx), W - x0), 0);
    const int y0 = min(max(vy_min[r0 + i] - lo, 0), max(nrows - 1, 0));
    ymin[i] = y0;
    ylen[i] = max(min(min(vy_len[r0 + i], ky), nrows - y0), 0);
  }
  __syncthreads();

  // horizontal pass: stage[r][px][c] for the input rows lo .. lo + nrows
  const uint8_t* frame = frames + (size_t)n * H * W * 3;
  const int P3 = P * 3;
  for (int i = tid; i < nrows * P3; i += F2P_THREADS) {
    const int r = i / P3, pc = i - r * P3;
    const int px = pc / 3, c = pc - px * 3;
    const uint8_t* src = frame + ((size_t)(lo + r) * W + xmin[px]) * 3 + c;
    const int32_t* w = wx + px * kx;
    int acc = 1 << (F2P_PB - 1);
    const int len = xlen[px];
    for (int t = 0; t < len; t++) acc += (int)src[t * 3] * w[t];
    stage[i] = (uint8_t)clip8(acc);
  }
  __syncthreads();

  // vertical pass on the uint8 rows: res[py][px][c]
  for (int i = tid; i < P * P3; i += F2P_THREADS) {
    const int py = i / P3, pc = i - py * P3;
    const uint8_t* src = stage + ymin[py] * P3 + pc;
    const int32_t* w = wy + py * ky;
    int acc = 1 << (F2P_PB - 1);
    const int len = ylen[py];
    for (int t = 0; t < len; t++) acc += (int)src[t * P3] * w[t];
    res[i] = (uint8_t)clip8(acc);
  }
  __syncthreads();

  // lookup and 16-byte stores: VEC consecutive px of one (c, py)
  constexpr int VEC = 16 / (int)sizeof(T);
  struct alignas(16) Vec { T v[VEC]; };
  const int pv = P / VEC;
  T* orow = out + (size_t)patch * 3 * P * P;
  for (int i = tid; i < 3 * P * pv; i += F2P_THREADS) {
    const int c = i / (P * pv), rem = i - c * (P * pv);
    const int py = rem / pv, px0 = (rem - py * pv) * VEC;
    const T* l = lut + c * 256;
    Vec o;
#pragma unroll
    for (int j = 0; j < VEC; j++) o.v[j] = l[res[(py * P + px0 + j) * 3 + c]];
    *reinterpret_cast<Vec*>(orow + (size_t)c * P * P + py * P + px0) = o;
  }
  if (crop) {
    // P * 3 consecutive bytes per image row; 4 bytes per store (P is a multiple of 8, R * 3 and c0 * 3 are multiples of 4)
    const int q = P3 / 4;
    for (int i = tid; i < P * q; i += F2P_THREADS) {
      const int py = i / q, b = (i - py * q) * 4;
      const uint32_t v = *reinterpret_cast<const uint32_t*>(res + py * P3 + b);
      *reinterpret_cast<uint32_t*>(crop + (((size_t)n * R + r0 + py) * R + c0) * 3 + b) = v;
    }
  }
}

// x[n * L + l] = ln_pre(l == 0 ? cls + pos[0] : e[n * (L - 1) + l - 1] + pos[l])
__global__ __launch_bounds__(256) void vit_embed_kernel(int M, int L, int d, const float* __restrict__ e, const float* __restrict__ cls,
                                                        const float* __restrict__ pos, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, float* __restrict__ x) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;   // whole waves leave: no shuffle below runs with missing lanes
  const int n = row / L, l = row - n * L;
  const float* a = l == 0 ? cls : e + ((size_t)n * (L - 1) + (l - 1)) * d;
  const float* p = pos + (size_t)l * d;
  const int nvec = d >> 2;
  float s[TXT_MAXIT][4];
  float sum = 0.0f;
#pragma unroll
  for (int it = 0; it < TXT_MAXIT; it++) {
    const int vi = it * 64 + lane;
    if (vi < nvec) {
      const float4 v = *reinterpret_cast<const float4*>(a + vi * 4);
      const float4 q = *reinterpret_cast<const float4*>(p + vi * 4);
      s[it][0] = v.x + q.x; s[it][1] = v.y + q.y; s[it][2] = v.z + q.z; s[it][3] = v.w + q.w;
      sum += (s[it][0] + s[it][1]) + (s[it][2] + s[it][3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; j++) s[it][j] = 0.0f;
    }
  }
  ln_regs<float>(s, sum, gamma, beta, x + (size_t)row * d, d, lane);
}

template <typename T>
__global__ __launch_bounds__(256) void vit_pool_kernel(int N, int L, int d, const float* __restrict__ x, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, T* __restrict__ y) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;
  ln_row<T>(x + (size_t)n * L * d, gamma, beta, y + (size_t)n * d, d, lane);
}

}  // namespace vct

using namespace vct;

extern "C" int vct_frames_to_patches(int out_dtype, int N, int H, int W, int R, int P, const uint8_t* frames, const int32_t* hx_min,
                                     const int32_t* hx_len, const int32_t* hx_w, int kx, const int32_t* vy_min, const int32_t* vy_len,
                                     const int32_t* vy_w, int ky, int stage_rows, const void* lut, void* out, uint8_t* crop,
                                     void* stream) {
  if (!frames || !hx_min || !hx_len || !hx_w || !vy_min || !vy_len || !vy_w || !lut || !out) return VCT_E_ARG;
  if (out_dtype != VCT_F32 && out_dtype != VCT_BF16) return VCT_E_ARG;
  if (N < 1 || H < 1 || W < 1 || R < 1 || P < 1 || kx < 1 || ky < 1 || stage_rows < 1) return VCT_E_SHAPE;
  if (R % P) return VCT_E_SHAPE;
  if (P % 8) return VCT_E_ALIGN;    // 16-byte stores of 8 bf16 / 4 fp32 along px, 4-byte stores into the crop
  const long long G = R / P;
  if (kx > W || ky > H || stage_rows > H) return VCT_E_SHAPE;
  if ((long long)N * G * G > 0x7fffffffLL || (long long)H * W > 0x7fffffffLL / 3) return VCT_E_SHAPE;
  const long long lds = f2p_lds_bytes(P, kx, ky, stage_rows);
  if (lds > F2P_LDS_MAX) return VCT_E_SHAPE;   // the window is too large for the staging
  if ((((uintptr_t)hx_min | (uintptr_t)hx_len | (uintptr_t)hx_w | (uintptr_t)vy_min | (uintptr_t)vy_len | (uintptr_t)vy_w) & 3)) return VCT_E_ALIGN;
  if (((uintptr_t)out & 15) || ((uintptr_t)lut & (out_dtype == VCT_BF16 ? 1 : 3)) || ((uintptr_t)crop & 3)) return VCT_E_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)(N * G * G));
  if (out_dtype == VCT_BF16)
    vct::launch((frames_to_patches_kernel<bf16_t>), grid, dim3(F2P_THREADS), (size_t)lds, st, H, W, R, P, (int)G, frames, hx_min, hx_len,
                hx_w, kx, vy_min, vy_len, vy_w, ky, stage_rows, (const bf16_t*)lut, (bf16_t*)out, crop);
  else
    vct::launch((frames_to_patches_kernel<float>), grid, dim3(F2P_THREADS), (size_t)lds, st, H, W, R, P, (int)G, frames, hx_min, hx_len,
                hx_w, kx, vy_min, vy_len, vy_w, ky, stage_rows, (const float*)lut, (float*)out, crop);
  VCT_CHECK_LAUNCH();
  return VCT_OK;
}

extern "C" int vct_vit_embed(int N, int L, int d, const float* e, const float* cls, const float* pos, const float* gamma,
                             const float* beta, float* x, void* stream) {
  if (!e || !cls || !pos || !gamma || !beta || !x) return VCT_E_ARG;
  const int rc = ln_row_check(VCT_F32, d);
  if (rc) return rc;
  if (N < 1 || L < 2 || (long long)N * L > 0x7fffffffLL) return VCT_E_SHAPE;
  if (((uintptr_t)e | (uintptr_t)cls | (uintptr_t)pos | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)x) & 15) return VCT_E_ALIGN;
  const int M = N * L;
  vct::launch(vit_embed_kernel, dim3((M + 3) / 4), dim3(256), 0, (hipStream_t)stream, M, L, d, e, cls, pos, gamma, beta, x);
  VCT_CHECK_LAUNCH();
  return VCT_OK;
}

extern "C" int vct_vit_pool(int out_dtype, int N, int L, int d, const float* x, const float* gamma, const float* beta, void* y,
                            void* stream) {
  if (!x || !gamma || !beta || !y) return VCT_E_ARG;
  const int rc = ln_row_check(out_dtype, d);
  if (rc) return rc;
  if (N < 1 || L < 1) return VCT_E_SHAPE;
  if (((uintptr_t)x | (uintptr_t)gamma | (uintptr_t)beta) & 15) return VCT_E_ALIGN;
  if ((uintptr_t)y & (out_dtype == VCT_BF16 ? 7 : 15)) return VCT_E_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  if (out_dtype == VCT_BF16)
    vct::launch((vit_pool_kernel<bf16_t>), dim3((N + 3) / 4), dim3(256), 0, st, N, L, d, x, gamma, beta, (bf16_t*)y);
  else
    vct::launch((vit_pool_kernel<float>), dim3((N + 3) / 4), dim3(256), 0, st, N, L, d, x, gamma, beta, (float*)y);
  VCT_CHECK_LAUNCH();
  return VCT_OK;
}
