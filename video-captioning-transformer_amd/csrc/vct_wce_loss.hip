// Self-critical sequence training on gfx950: the sequence-weighted cross-entropy with its logits gradient and per-token
// log-probabilities (vct_wce_loss), and the group sum that folds the decoder's d(memory) of N samples per video back onto the
// video (vct_group_sum).  The loss kernel is sce_loss_kernel (vct_elem.hip) at alpha = 1 with one more factor in the per-row
// scalar: same launch shapes, same operation order, so unit weights reproduce vct_sce_loss(alpha = 1) bit for bit.
#include "vct_common.h"

namespace vct {

template <typename T> struct WV { static constexpr int VEC = 16 / sizeof(T); };
template <typename T, int VEC> struct alignas(sizeof(T) * VEC) WPack { T v[VEC]; };

// fixed-order count of the valid rows: one workgroup, no atomics
__global__ void wce_count_kernel(int N, int S, const int64_t* __restrict__ labels, int64_t lbstride, int64_t pad_id,
                                 float* __restrict__ out) {
  __shared__ float red[16];
  float c = 0.0f;
  for (int n = threadIdx.x; n < N; n += blockDim.x) c += (labels[(size_t)(n / S) * lbstride + (n % S)] != pad_id) ? 1.0f : 0.0f;
  c = block_sum<16>(c, red);
  if (threadIdx.x == 0) out[0] = c;
}

// One NT-thread workgroup per row; the row lives in REGISTERS (IT 16-byte vectors per thread, loaded once), LDS only carries the
// two block reductions (one array and ONE barrier each).  `one` is 1.0f, passed as an argument so that the per-row scalar is the
// same runtime division vct_sce_loss does with its alpha.
template <typename T, int IT, int NT>
__global__ __launch_bounds__(NT, NT / 128) void wce_loss_kernel(int N, int S, int V, const T* __restrict__ logits, int64_t ldl,
                                                        const int64_t* __restrict__ labels, int64_t lbstride, int64_t pad_id,
                                                        float one, const float* __restrict__ seq_w, float* __restrict__ tok_logp,
                                                        T* __restrict__ dlogits, int64_t ld_dl, float* __restrict__ row_ws) {
  __shared__ float red_m[16], red_s[16];
  constexpr int VEC = WV<T>::VEC, NW = NT / 64;
  using P = WPack<T, VEC>;
  const int n = blockIdx.x, tid = threadIdx.x, wv = tid >> 6, ln = tid & 63;
  const T* x = logits + (size_t)n * ldl;
  const int b = n / S;
  const int64_t y_in = labels[(size_t)b * lbstride + (n % S)];
  const bool valid = (y_in != pad_id);
  // a label outside the vocabulary: computed against column 0 (no stray access); a valid row poisons the loss with NaN
  const bool oob = (y_in < 0 || y_in >= V);
  const int64_t y = oob ? 0 : y_in;
  const float nvalid = row_ws[2 * N];
  const float w = (seq_w != nullptr) ? seq_w[b] : 1.0f;
  const float xy = to_f<T>(x[y]);
  const int nv = (V + VEC - 1) / VEC;                 // vectors holding valid columns (ldl covers the rounded-up row)
  P pk[IT];
#pragma unroll
  for (int it = 0; it < IT; it++) pk[it] = *reinterpret_cast<const P*>(x + (size_t)min(it * NT + tid, nv - 1) * VEC);
  float e[IT][VEC];
  float mx = -INFINITY;
#pragma unroll
  for (int it = 0; it < IT; it++) {
    const int vi = it * NT + tid;
#pragma unroll
    for (int j = 0; j < VEC; j++) e[it][j] = to_f<T>(pk[it].v[j]);
    if (vi >= nv - 1) {                                // only the last vector of the row (and beyond) needs masking
#pragma unroll
      for (int j = 0; j < VEC; j++)
        if (vi >= nv || vi * VEC + j >= V) e[it][j] = -INFINITY;
    }
#pragma unroll
    for (int j = 0; j < VEC; j++) mx = fmaxf(mx, e[it][j]);
  }
  mx = wave_max(mx);
  if (ln == 0) red_m[wv] = mx;
  __syncthreads();
  mx = red_m[0];
#pragma unroll
  for (int i = 1; i < NW; i++) mx = fmaxf(mx, red_m[i]);
  float se = 0.0f;
#pragma unroll
  for (int it = 0; it < IT; it++)
#pragma unroll
    for (int j = 0; j < VEC; j++) { e[it][j] = __expf(e[it][j] - mx); se += e[it][j]; }   // padding: exp(-inf) = 0
  se = wave_sum(se);
  if (ln == 0) red_s[wv] = se;
  __syncthreads();
  se = 0.0f;
#pragma unroll
  for (int i = 0; i < NW; i++) se += red_s[i];
  const float inv = 1.0f / se;
  const float py = __expf(xy - mx) * inv;
  if (tid == 0) {
    const float nll = (mx + __logf(se)) - xy;         // -log p(label)
    row_ws[n] = valid ? (oob ? __builtin_nanf("") : w * nll) : 0.0f;
    // (the definition's order: x[y] - max is exact or nearly so, which keeps a log-probability near 0 accurate)
    if (tok_logp != nullptr) tok_logp[n] = valid ? (oob ? __builtin_nanf("") : (xy - mx) - __logf(se)) : 0.0f;
  }
  if (dlogits == nullptr) return;
  const float a = valid ? (one / nvalid) * w : 0.0f;   // pad rows: p_j * 0 = exact zeros
  T* dx = dlogits + (size_t)n * ld_dl;
  const int nvo = (int)(ld_dl / VEC);
#pragma unroll
  for (int it = 0; it < IT; it++) {
    const int vi = it * NT + tid;
    if (vi < nvo) {
      P o;
#pragma unroll
      for (int j = 0; j < VEC; j++) {
        const float pj = e[it][j] * inv;
        o.v[j] = from_f<T>(pj * a);
      }
      *reinterpret_cast<P*>(dx + vi * VEC) = o;
    }
  }
  // the label column: a * (p_y - 1)   (written after the row's vector stores)
  __syncthreads();
  if (tid == 0) dx[y] = from_f<T>(a * (py - 1.0f));
}

// loss = (sum of the rows' weighted terms) / count: one workgroup, fixed order
__global__ void wce_finalize_kernel(int N, const float* __restrict__ row_ws, float* __restrict__ loss) {
  __shared__ float red[16];
  float ce = 0.0f;
  for (int n = threadIdx.x; n < N; n += blockDim.x) ce += row_ws[n];
  ce = block_sum<16>(ce, red);
  if (threadIdx.x == 0) loss[0] = ce / row_ws[2 * N];
}

// out[(g*R + r), :] = sum over n < G (ascending, fp32) of in[((g*G + n)*R + r), :]; one thread per 16-byte vector of `out`.
// The first term initialises the accumulator, so G = 1 copies bit for bit (-0 stays -0).
template <typename T>
__global__ __launch_bounds__(256) void group_sum_kernel(int64_t nvec_out, int G, int R, int dv, const T* __restrict__ in,
                                                        T* __restrict__ out) {
  constexpr int VEC = WV<T>::VEC;
  using P = WPack<T, VEC>;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nvec_out) return;
  const int64_t row = i / dv, c = i - row * dv;         // output row g*R + r, vector column c
  const int64_t g = row / R, r = row - g * R;
  const P* src = reinterpret_cast<const P*>(in) + ((g * G) * R + r) * dv + c;
  const int64_t step = (int64_t)R * dv;                  // vectors between two blocks of a group
  if (G == 1) {
    reinterpret_cast<P*>(out)[i] = src[0];
    return;
  }
  float acc[VEC];
  const P v0 = src[0];
#pragma unroll
  for (int j = 0; j < VEC; j++) acc[j] = to_f<T>(v0.v[j]);
  for (int n = 1; n < G; n++) {
    const P v = src[n * step];
#pragma unroll
    for (int j = 0; j < VEC; j++) acc[j] += to_f<T>(v.v[j]);
  }
  P o;
#pragma unroll
  for (int j = 0; j < VEC; j++) o.v[j] = from_f<T>(acc[j]);
  reinterpret_cast<P*>(out)[i] = o;
}

}  // namespace vct

using namespace vct;

static bool wce_dt_ok(int dt) { return dt == VCT_F32 || dt == VCT_BF16; }
static int wce_vec_of(int dt) { return dt == VCT_BF16 ? 8 : 4; }

extern "C" int vct_wce_loss(int dtype, int N, int S, int V, const void* logits, int64_t ldl, const int64_t* labels,
                            int64_t label_batch_stride, int64_t pad_id, const float* seq_w, float* loss_out, float* tok_logp,
                            void* dlogits, int64_t ld_dl, float* row_ws, void* stream) {
  if (!wce_dt_ok(dtype) || !logits || !labels || !loss_out || !row_ws) return VCT_E_ARG;
  if (N <= 0 || S <= 0 || V <= 0 || N % S) return VCT_E_SHAPE;
  const int vec = wce_vec_of(dtype);
  const int64_t vround = ((int64_t)V + vec - 1) / vec * vec;
  if (ldl < vround || ldl % vec || ((uintptr_t)logits & 15)) return VCT_E_ALIGN;       // rows are read as 16-byte vectors
  if (dlogits && (ld_dl < vround || ld_dl % vec || ((uintptr_t)dlogits & 15))) return VCT_E_ALIGN;
  if ((dlogits && ld_dl > (int64_t)8 * 1024 * vec) || vround > (int64_t)8 * 1024 * vec) return VCT_E_SHAPE;   // row must fit the register tile
  hipStream_t st = (hipStream_t)stream;
  vct::launch(wce_count_kernel, dim3(1), dim3(1024), 0, st, N, S, labels, label_batch_stride, pad_id, row_ws + 2 * (size_t)N);
  VCT_CHECK_LAUNCH();
  const int64_t width = dlogits ? (ld_dl > vround ? ld_dl : vround) : vround;
  const bool small = width <= (int64_t)4 * 1024 * vec;
#define VCT_WCE(T_, IT_, NT_) vct::launch((wce_loss_kernel<T_, IT_, NT_>), dim3(N), dim3(NT_), 0, st, N, S, V, (const T_*)logits, ldl, \
                                          labels, label_batch_stride, pad_id, 1.0f, seq_w, tok_logp, (T_*)dlogits, ld_dl, row_ws)
  // vct_sce_loss's launch shapes (measured there at V = 30522)
  if (dtype == VCT_BF16) { if (small) VCT_WCE(bf16_t, 8, 512); else VCT_WCE(bf16_t, 8, 1024); }
  else { if (small) VCT_WCE(float, 4, 1024); else VCT_WCE(float, 8, 1024); }
#undef VCT_WCE
  VCT_CHECK_LAUNCH();
  vct::launch(wce_finalize_kernel, dim3(1), dim3(1024), 0, st, N, (const float*)row_ws, loss_out);
  VCT_CHECK_LAUNCH();
  return VCT_OK;
}

extern "C" int vct_group_sum(int dtype, int B, int G, int R, int d, const void* in, void* out, void* stream) {
  if (!wce_dt_ok(dtype) || !in || !out) return VCT_E_ARG;
  const int vec = wce_vec_of(dtype);
  if (B <= 0 || G <= 0 || R <= 0 || d <= 0 || d % vec) return VCT_E_SHAPE;
  if (((uintptr_t)in & 15) || ((uintptr_t)out & 15)) return VCT_E_ALIGN;
  const int dv = d / vec;
  const int64_t nvec_out = (int64_t)B * R * dv;
  const int64_t blocks = (nvec_out + 255) / 256;
  if (blocks > 0x7fffffffLL || (int64_t)B * G * R > 0x7fffffffLL) return VCT_E_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == VCT_BF16) vct::launch(group_sum_kernel<bf16_t>, dim3((unsigned)blocks), dim3(256), 0, st, nvec_out, G, R, dv, (const bf16_t*)in, (bf16_t*)out);
  else vct::launch(group_sum_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, st, nvec_out, G, R, dv, (const float*)in, (float*)out);
  VCT_CHECK_LAUNCH();
  return VCT_OK;
}
