// Label-smoothed symmetric cross-entropy on gfx950 (vct_sce_loss_ls): sce_loss_kernel (vct_elem.hip) with the smoothed CE term
//   ce_n = (1 - eps) * nll_n + eps * (lse - mean_j x_j)
// and two by-products per row, the un-smoothed NLL and whether the label's logit is the row maximum.  Same launch shapes and,
// for everything the two kernels share, the same operation order: eps = 0 reproduces vct_sce_loss's loss and gradient bit for bit
// (the new terms are exact zeros there).  The RCE term is not smoothed.
#include "vct_common.h"

namespace vct {

template <typename T> struct LV { static constexpr int VEC = 16 / sizeof(T); };
template <typename T, int VEC> struct alignas(sizeof(T) * VEC) LPack { T v[VEC]; };

constexpr float LS_SCE_C = 9.210340371976184f;  // -log(1e-4): sce_loss_kernel's SCE_C

// fixed-order count of the valid rows: one workgroup, no atomics
__global__ void ls_count_kernel(int N, int S, const int64_t* __restrict__ labels, int64_t lbstride, int64_t pad_id,
                                float* __restrict__ out) {
  __shared__ float red[16];
  float c = 0.0f;
  for (int n = threadIdx.x; n < N; n += blockDim.x) c += (labels[(size_t)(n / S) * lbstride + (n % S)] != pad_id) ? 1.0f : 0.0f;
  c = block_sum<16>(c, red);
  if (threadIdx.x == 0) out[0] = c;
}

// One NT-thread workgroup per row; the row lives in REGISTERS (IT 16-byte vectors per thread, loaded once), LDS only carries the
// block reductions.  The row sum of x for the smoothing term is taken over the VALID columns only -- the masked lanes hold -inf
// for the maximum and columns V..ldl-1 may hold anything -- per thread over (it, j), then the wave, then the waves in index
// order; its partials cross the barrier of the maximum, so the kernel has sce_loss_kernel's barriers and no more.
// row_ws: [0, N) smoothed CE rows, [N, 2N) RCE rows, [2N] count, [2N + 1, 3N + 1) NLL rows, [3N + 1, 4N + 1) hit rows.
template <typename T, int IT, int NT>
__global__ __launch_bounds__(NT, NT / 128) void sce_ls_kernel(int N, int S, int V, const T* __restrict__ logits, int64_t ldl,
                                                      const int64_t* __restrict__ labels, int64_t lbstride, int64_t pad_id,
                                                      float alpha, float eps, T* __restrict__ dlogits, int64_t ld_dl,
                                                      float* __restrict__ row_ws) {
  __shared__ float red_m[16], red_x[16], red_s[16], red_q[16], red_c[16];
  constexpr int VEC = LV<T>::VEC, NW = NT / 64;
  using P = LPack<T, VEC>;
  const int n = blockIdx.x, tid = threadIdx.x, wv = tid >> 6, ln = tid & 63;
  const T* x = logits + (size_t)n * ldl;
  const int64_t y_in = labels[(size_t)(n / S) * lbstride + (n % S)];
  const bool valid = (y_in != pad_id);
  // a label outside the vocabulary: computed against column 0 (no stray access); a valid row poisons loss and NLL with NaN
  const bool oob = (y_in < 0 || y_in >= V);
  const int64_t y = oob ? 0 : y_in;
  const float nvalid = row_ws[2 * N];
  const float xy = to_f<T>(x[y]);
  const int nv = (V + VEC - 1) / VEC;                 // vectors holding valid columns (ldl covers the rounded-up row)
  P pk[IT];
#pragma unroll
  for (int it = 0; it < IT; it++) pk[it] = *reinterpret_cast<const P*>(x + (size_t)min(it * NT + tid, nv - 1) * VEC);
  float e[IT][VEC];
  float mx = -INFINITY, sx = 0.0f;
#pragma unroll
  for (int it = 0; it < IT; it++) {
    const int vi = it * NT + tid;
#pragma unroll
    for (int j = 0; j < VEC; j++) e[it][j] = to_f<T>(pk[it].v[j]);
    if (vi >= nv - 1) {                                // only the last vector of the row (and beyond) needs masking
#pragma unroll
      for (int j = 0; j < VEC; j++) {
        if (vi >= nv || vi * VEC + j >= V) e[it][j] = -INFINITY;
        else sx += e[it][j];                           // a masked lane never reaches the sum (a select, not a product with 0)
      }
    } else {
#pragma unroll
      for (int j = 0; j < VEC; j++) sx += e[it][j];
    }
#pragma unroll
    for (int j = 0; j < VEC; j++) mx = fmaxf(mx, e[it][j]);
  }
  mx = wave_max(mx);
  sx = wave_sum(sx);
  if (ln == 0) { red_m[wv] = mx; red_x[wv] = sx; }
  __syncthreads();
  mx = red_m[0];
#pragma unroll
  for (int i = 1; i < NW; i++) mx = fmaxf(mx, red_m[i]);
  sx = 0.0f;
#pragma unroll
  for (int i = 0; i < NW; i++) sx += red_x[i];
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
  const float beta = 1.0f - alpha;
  const float py = __expf(xy - mx) * inv;
  // the RCE term, exactly sce_loss_kernel's (never smoothed)
  float q = 0.0f, cnt = 0.0f;
  if (alpha != 1.0f) {
#pragma unroll
    for (int it = 0; it < IT; it++)
#pragma unroll
      for (int j = 0; j < VEC; j++) {
        const float pj = e[it][j] * inv;
        const bool big = pj >= 1e-7f;
        q += big ? pj : 0.0f;
        cnt += big ? 0.0f : 1.0f;
      }
    q = wave_sum(q);
    cnt = wave_sum(cnt);
    if (ln == 0) { red_q[wv] = q; red_c[wv] = cnt; }
    __syncthreads();
    q = 0.0f; cnt = 0.0f;
#pragma unroll
    for (int i = 0; i < NW; i++) { q += red_q[i]; cnt += red_c[i]; }
    cnt -= (float)(IT * NT * VEC - V);                 // masked / padding slots were counted as "small"
    if (py >= 1e-7f) q -= py; else cnt -= 1.0f;        // remove the label column
  }
  if (tid == 0) {
    const float lse = mx + __logf(se);
    const float nll = lse - xy;
    float ce = nll;
    if (eps != 0.0f) ce = (1.0f - eps) * nll + eps * (lse - sx / (float)V);
    const float nan = __builtin_nanf("");
    row_ws[n] = valid ? (oob ? nan : ce) : 0.0f;
    row_ws[N + n] = LS_SCE_C * (q + 1e-7f * cnt);
    row_ws[2 * (size_t)N + 1 + n] = valid ? (oob ? nan : nll) : 0.0f;
    row_ws[3 * (size_t)N + 1 + n] = (valid && !oob && xy == mx) ? 1.0f : 0.0f;   // a tie with the maximum is a hit
  }
  if (dlogits == nullptr) return;
  // off the label:  p_j * (a + bn*(G_j - c*Q)) - a*eps/V;  columns V..ld_dl-1 are zeros
  const float a = valid ? alpha / nvalid : 0.0f;
  const float bn = (alpha != 1.0f) ? beta / (float)N : 0.0f;
  const float k_small = a - bn * LS_SCE_C * q;         // multiplier when p_j <  1e-7
  const float k_big = k_small + bn * LS_SCE_C;         // multiplier when p_j >= 1e-7
  const float sm = a * eps / (float)V;                 // exact 0 at eps = 0 and on pad rows
  const float om = 1.0f - eps;
  T* dx = dlogits + (size_t)n * ld_dl;
  const int nvo = (int)(ld_dl / VEC);
#pragma unroll
  for (int it = 0; it < IT; it++) {
    const int vi = it * NT + tid;
    if (vi < nvo) {
      float g[VEC];
#pragma unroll
      for (int j = 0; j < VEC; j++) {
        const float pj = e[it][j] * inv;
        g[j] = pj * (pj >= 1e-7f ? k_big : k_small);
      }
      if (vi >= nv - 1) {                              // the constant must not reach the columns behind V: they keep p_j * k = 0
#pragma unroll
        for (int j = 0; j < VEC; j++)
          if (!(vi >= nv || vi * VEC + j >= V)) g[j] -= sm;
      } else {
#pragma unroll
        for (int j = 0; j < VEC; j++) g[j] -= sm;
      }
      P o;
#pragma unroll
      for (int j = 0; j < VEC; j++) o.v[j] = from_f<T>(g[j]);
      *reinterpret_cast<P*>(dx + vi * VEC) = o;
    }
  }
  // the label column: a*(p_y - (1 - eps)) + bn*p_y*(0 - c*Q) - a*eps/V   (written after the row's vector stores)
  __syncthreads();
  if (tid == 0) {
    const float gy = a * (py - om) - bn * py * LS_SCE_C * q;
    dx[y] = from_f<T>(gy - sm);
  }
}

// one workgroup, fixed order: loss as sce_finalize_kernel; stats = (sum nll / count, sum hit / count)
__global__ void sce_ls_finalize_kernel(int N, float alpha, const float* __restrict__ row_ws, float* __restrict__ loss,
                                       float* __restrict__ stats) {
  __shared__ float red[16];
  float ce = 0.0f, rce = 0.0f;
  for (int n = threadIdx.x; n < N; n += blockDim.x) { ce += row_ws[n]; rce += row_ws[N + n]; }
  ce = block_sum<16>(ce, red);
  rce = block_sum<16>(rce, red);
  const float nvalid = row_ws[2 * N];
  if (threadIdx.x == 0) {
    const float l_ce = ce / nvalid;
    loss[0] = (alpha == 1.0f) ? l_ce : alpha * l_ce + (1.0f - alpha) * (rce / (float)N);
  }
  if (stats == nullptr) return;
  float nll = 0.0f, hit = 0.0f;
  const float* rn = row_ws + 2 * (size_t)N + 1;
  const float* rh = row_ws + 3 * (size_t)N + 1;
  for (int n = threadIdx.x; n < N; n += blockDim.x) { nll += rn[n]; hit += rh[n]; }
  nll = block_sum<16>(nll, red);
  hit = block_sum<16>(hit, red);
  if (threadIdx.x == 0) { stats[0] = nll / nvalid; stats[1] = hit / nvalid; }
}

}  // namespace vct

using namespace vct;

extern "C" int vct_sce_loss_ls(int dtype, int N, int S, int V, const void* logits, int64_t ldl, const int64_t* labels,
                               int64_t label_batch_stride, int64_t pad_id, float alpha, float smoothing, float* loss_out,
                               float* stats_out, void* dlogits, int64_t ld_dl, float* row_ws, void* stream) {
  if ((dtype != VCT_F32 && dtype != VCT_BF16) || !logits || !labels || !loss_out || !row_ws) return VCT_E_ARG;
  if (!(smoothing >= 0.0f && smoothing < 1.0f)) return VCT_E_ARG;       // NaN fails both comparisons
  if (N <= 0 || S <= 0 || V <= 0 || N % S) return VCT_E_SHAPE;
  const int vec = dtype == VCT_BF16 ? 8 : 4;
  const int64_t vround = ((int64_t)V + vec - 1) / vec * vec;
  if (ldl < vround || ldl % vec || ((uintptr_t)logits & 15)) return VCT_E_ALIGN;       // rows are read as 16-byte vectors
  if (dlogits && (ld_dl < vround || ld_dl % vec || ((uintptr_t)dlogits & 15))) return VCT_E_ALIGN;
  if (ld_dl > (int64_t)8 * 1024 * vec || vround > (int64_t)8 * 1024 * vec) return VCT_E_SHAPE;   // row must fit the register tile
  hipStream_t st = (hipStream_t)stream;
  vct::launch(ls_count_kernel, dim3(1), dim3(1024), 0, st, N, S, labels, label_batch_stride, pad_id, row_ws + 2 * (size_t)N);
  VCT_CHECK_LAUNCH();
  const int64_t width = dlogits ? (ld_dl > vround ? ld_dl : vround) : vround;
  const bool small = width <= (int64_t)4 * 1024 * vec;
#define VCT_SCE_LS(T_, IT_, NT_) vct::launch((sce_ls_kernel<T_, IT_, NT_>), dim3(N), dim3(NT_), 0, st, N, S, V, (const T_*)logits, ldl, \
                                             labels, label_batch_stride, pad_id, alpha, smoothing, (T_*)dlogits, ld_dl, row_ws)
  // vct_sce_loss's launch shapes (measured there at V = 30522)
  if (dtype == VCT_BF16) { if (small) VCT_SCE_LS(bf16_t, 8, 512); else VCT_SCE_LS(bf16_t, 8, 1024); }
  else { if (small) VCT_SCE_LS(float, 4, 1024); else VCT_SCE_LS(float, 8, 1024); }
#undef VCT_SCE_LS
  VCT_CHECK_LAUNCH();
  vct::launch(sce_ls_finalize_kernel, dim3(1), dim3(1024), 0, st, N, alpha, (const float*)row_ws, loss_out, stats_out);
  VCT_CHECK_LAUNCH();
  return VCT_OK;
}
