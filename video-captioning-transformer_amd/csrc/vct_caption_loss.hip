// The caption losses over the vocabulary logits on gfx950 -- one kernel family, three entry points -- and the per-video sum of
// sampled rows (vct_group_sum):
//   vct_sce_loss     SCE   symmetric cross-entropy: alpha * CE + (1 - alpha) * RCE
//   vct_sce_loss_ls  LS    SCE with label smoothing on the CE term,  ce_n = (1 - eps) * nll_n + eps * (lse - mean_j x_j),  and two
//                          by-products per row: the un-smoothed NLL and whether the label's logit is the row maximum.  RCE is not smoothed
//   vct_wce_loss     WCE   sequence-weighted CE (self-critical training) with the per-token log-probabilities; no RCE term
// Each call is three launches: count_valid_kernel, sce_loss_kernel<T, IT, NT, KIND>, sce_finalize_kernel<KIND>.  The kinds are ONE
// algorithm; what a kind adds sits behind `if constexpr`, and everything the kinds share is one piece of source in one operation order.
// That is what the bitwise promises of include/vct_hip.h rest on: LS at eps = 0 writes vct_sce_loss's loss and gradient (the added
// terms are exact zeros there), WCE at unit weights writes vct_sce_loss(alpha = 1)'s.
// ld_dl is ignored when dlogits is NULL.
#include "vct_common.h"

namespace vct {

template <typename T> struct LV { static constexpr int VEC = 16 / sizeof(T); };
template <typename T, int VEC> struct alignas(sizeof(T) * VEC) LPack { T v[VEC]; };

enum LossKind { SCE = 0, LS = 1, WCE = 2 };

constexpr float SCE_C = 9.210340371976184f;  // -log(1e-4): loss.py:86-88 off-target log(clamp(onehot))

// fixed-order count of the valid rows: one workgroup, no atomics
__global__ void count_valid_kernel(int N, int S, const int64_t* __restrict__ labels, int64_t lbstride, int64_t pad_id,
                                   float* __restrict__ out) {
  __shared__ float red[16];
  float c = 0.0f;
  for (int n = threadIdx.x; n < N; n += blockDim.x) c += (labels[(size_t)(n / S) * lbstride + (n % S)] != pad_id) ? 1.0f : 0.0f;
  c = block_sum<16>(c, red);
  if (threadIdx.x == 0) out[0] = c;
}

// One NT-thread workgroup per row; the row lives in REGISTERS (IT 16-byte vectors per thread, loaded
// once from HBM), so every logit costs one HBM read, one exp and one HBM write (the gradient), and
// LDS only carries the block reductions.  NT*IT vectors must cover the row: 512 x 8 for bf16 rows up to 4096 vectors (measured best; 256 x 16: few waves per
// barrier, 16 loads in flight per thread, 3 rows per CU) or 1024 x 8 for very wide vocabularies.
// row_ws: [0, N) CE rows (LS: smoothed; WCE: weighted), [N, 2N) RCE rows (WCE: not written), [2N] count of valid rows;
//         LS only: [2N + 1, 3N + 1) NLL rows, [3N + 1, 4N + 1) hit rows.
// alpha: WCE is given 1.0f, as an argument, so that its per-row scalar is the runtime division SCE does with its alpha.
// eps (LS), seq_w and tok_logp (WCE) are read by their kind alone.
template <typename T, int IT, int NT, int KIND>
__global__ __launch_bounds__(NT, NT / 128) void sce_loss_kernel(int N, int S, int V, const T* __restrict__ logits, int64_t ldl,
                                                        const int64_t* __restrict__ labels, int64_t lbstride, int64_t pad_id,
                                                        float alpha, const float* __restrict__ seq_w, float* __restrict__ tok_logp,
                                                        T* __restrict__ dlogits, int64_t ld_dl, float* __restrict__ row_ws, float eps) {
  // one LDS array per block reduction: each costs ONE barrier (no guard barrier before reusing a shared scratch); an array no
  // kind of this instantiation touches takes no LDS
  __shared__ float red_m[16], red_x[16], red_s[16], red_q[16], red_c[16];
  constexpr int VEC = LV<T>::VEC, NW = NT / 64;
  using P = LPack<T, VEC>;
  const int n = blockIdx.x, tid = threadIdx.x, wv = tid >> 6, ln = tid & 63;
  const T* x = logits + (size_t)n * ldl;
  const int b = n / S;
  const int64_t y_in = labels[(size_t)b * lbstride + (n % S)];
  const bool valid = (y_in != pad_id);
  // a label outside the vocabulary (torch raises a device assert there) must not become a stray read / write: the row is
  // computed against column 0 and, when it counts towards the loss, poisons it (LS: and the NLL, WCE: and tok_logp) with NaN
  const bool oob = (y_in < 0 || y_in >= V);
  const int64_t y = oob ? 0 : y_in;
  const float nvalid = row_ws[2 * N];
  const float w = (KIND == WCE && seq_w != nullptr) ? seq_w[b] : 1.0f;
  const float xy = to_f<T>(x[y]);
  const int nv = (V + VEC - 1) / VEC;                 // vectors holding valid columns (ldl covers the rounded-up row)
  // all IT loads are issued back to back, unconditionally (index clamped, out-of-row vectors masked after)
  P pk[IT];
#pragma unroll
  for (int it = 0; it < IT; it++) pk[it] = *reinterpret_cast<const P*>(x + (size_t)min(it * NT + tid, nv - 1) * VEC);
  float e[IT][VEC];
  // LS: the row sum of x over the VALID columns only -- the masked lanes hold -inf for the maximum and columns V..ldl-1 may hold
  // anything -- per thread over (it, j), then the wave, then the waves in index order; its partials cross the barrier of the maximum
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
        else if constexpr (KIND == LS) sx += e[it][j];  // a masked lane never reaches the sum (a select, not a product with 0)
      }
    } else if constexpr (KIND == LS) {
#pragma unroll
      for (int j = 0; j < VEC; j++) sx += e[it][j];
    }
#pragma unroll
    for (int j = 0; j < VEC; j++) mx = fmaxf(mx, e[it][j]);
  }
  mx = wave_max(mx);
  if constexpr (KIND == LS) sx = wave_sum(sx);
  if (ln == 0) {
    red_m[wv] = mx;
    if constexpr (KIND == LS) red_x[wv] = sx;
  }
  __syncthreads();
  mx = red_m[0];
#pragma unroll
  for (int i = 1; i < NW; i++) mx = fmaxf(mx, red_m[i]);
  if constexpr (KIND == LS) {
    sx = 0.0f;
#pragma unroll
    for (int i = 0; i < NW; i++) sx += red_x[i];
  }
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
  // RCE (SCE, LS) over ALL columns: Qa = sum_{p_j >= 1e-7} p_j, ca = #{p_j < 1e-7} (padding has p = 0 and is counted: fixed below);
  // the label column is then taken out analytically -- no per-element (j != y) tests
  float q = 0.0f, cnt = 0.0f;
  if constexpr (KIND != WCE) {
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
      cnt -= (float)(IT * NT * VEC - V);               // masked / padding slots were counted as "small"
      if (py >= 1e-7f) q -= py; else cnt -= 1.0f;      // remove the label column
    }
  }
  if (tid == 0) {
    const float nan = __builtin_nanf("");
    if constexpr (KIND == SCE) row_ws[n] = valid ? (oob ? nan : (mx + __logf(se)) - xy) : 0.0f;
    if constexpr (KIND == LS) {
      const float lse = mx + __logf(se);
      const float nll = lse - xy;
      float ce = nll;
      if (eps != 0.0f) ce = (1.0f - eps) * nll + eps * (lse - sx / (float)V);
      row_ws[n] = valid ? (oob ? nan : ce) : 0.0f;
      row_ws[2 * (size_t)N + 1 + n] = valid ? (oob ? nan : nll) : 0.0f;
      row_ws[3 * (size_t)N + 1 + n] = (valid && !oob && xy == mx) ? 1.0f : 0.0f;   // a tie with the maximum is a hit
    }
    if constexpr (KIND == WCE) {
      const float nll = (mx + __logf(se)) - xy;         // -log p(label)
      row_ws[n] = valid ? (oob ? nan : w * nll) : 0.0f;
      // (the definition's order: x[y] - max is exact or nearly so, which keeps a log-probability near 0 accurate)
      if (tok_logp != nullptr) tok_logp[n] = valid ? (oob ? nan : (xy - mx) - __logf(se)) : 0.0f;
    }
    if constexpr (KIND != WCE) row_ws[N + n] = SCE_C * (q + 1e-7f * cnt);
  }
  if (dlogits == nullptr) return;
  // gradient for j != y.  SCE:  p_j * (a + bn*(G_j - c*Q)),  G_j = c*[p_j >= 1e-7];  LS: the same - a*eps/V on the columns below V;
  // WCE:  p_j * a.  Padding has p = 0 -> 0: columns V..ld_dl-1 are zeros, and so are pad rows (a = 0)
  const float a = valid ? (KIND == WCE ? (alpha / nvalid) * w : alpha / nvalid) : 0.0f;
  const float bn = (alpha != 1.0f) ? beta / (float)N : 0.0f;
  const float k_small = a - bn * SCE_C * q;            // multiplier when p_j <  1e-7
  const float k_big = k_small + bn * SCE_C;            // multiplier when p_j >= 1e-7
  const float sm = KIND == LS ? a * eps / (float)V : 0.0f;   // LS: exact 0 at eps = 0 and on pad rows
  const float om = KIND == LS ? 1.0f - eps : 1.0f;
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
        if constexpr (KIND == WCE) g[j] = pj * a;
        else g[j] = pj * (pj >= 1e-7f ? k_big : k_small);
      }
      if constexpr (KIND == LS) {
        if (vi >= nv - 1) {                            // the constant must not reach the columns behind V: they keep p_j * k = 0
#pragma unroll
          for (int j = 0; j < VEC; j++)
            if (!(vi >= nv || vi * VEC + j >= V)) g[j] -= sm;
        } else {
#pragma unroll
          for (int j = 0; j < VEC; j++) g[j] -= sm;
        }
      }
      P o;
#pragma unroll
      for (int j = 0; j < VEC; j++) o.v[j] = from_f<T>(g[j]);
      *reinterpret_cast<P*>(dx + vi * VEC) = o;
    }
  }
  // the label column (written after the row's vector stores).  SCE: a*(p_y - 1) + bn*p_y*(0 - c*Q);  LS: a*(p_y - (1 - eps)) + the
  // same - a*eps/V;  WCE: a*(p_y - 1)
  __syncthreads();
  if (tid == 0) {
    float gy = a * (py - om);
    if constexpr (KIND != WCE) gy -= bn * py * SCE_C * q;
    if constexpr (KIND == LS) gy -= sm;
    dx[y] = from_f<T>(gy);
  }
}

// one workgroup, fixed order: loss = CE / count (WCE), alpha * that + (1 - alpha) * mean RCE (SCE, LS; alpha = 1: CE alone);
// LS with stats: stats = (sum nll / count, sum hit / count)
template <int KIND>
__global__ void sce_finalize_kernel(int N, float alpha, const float* __restrict__ row_ws, float* __restrict__ loss,
                                    float* __restrict__ stats) {
  __shared__ float red[16];
  float ce = 0.0f, rce = 0.0f;
  for (int n = threadIdx.x; n < N; n += blockDim.x) {
    ce += row_ws[n];
    if constexpr (KIND != WCE) rce += row_ws[N + n];
  }
  ce = block_sum<16>(ce, red);
  if constexpr (KIND != WCE) rce = block_sum<16>(rce, red);
  const float nvalid = row_ws[2 * N];
  if (threadIdx.x == 0) {
    const float l_ce = ce / nvalid;
    if constexpr (KIND == WCE) loss[0] = l_ce;
    else loss[0] = (alpha == 1.0f) ? l_ce : alpha * l_ce + (1.0f - alpha) * (rce / (float)N);
  }
  if constexpr (KIND == LS) {
    if (stats == nullptr) return;
    float nll = 0.0f, hit = 0.0f;
    const float* rn = row_ws + 2 * (size_t)N + 1;
    const float* rh = row_ws + 3 * (size_t)N + 1;
    for (int n = threadIdx.x; n < N; n += blockDim.x) { nll += rn[n]; hit += rh[n]; }
    nll = block_sum<16>(nll, red);
    hit = block_sum<16>(hit, red);
    if (threadIdx.x == 0) { stats[0] = nll / nvalid; stats[1] = hit / nvalid; }
  }
}

// out[(g*R + r), :] = sum over n < G (ascending, fp32) of in[((g*G + n)*R + r), :]; one thread per 16-byte vector of `out`.
// The first term initialises the accumulator, so G = 1 copies bit for bit (-0 stays -0).
template <typename T>
__global__ __launch_bounds__(256) void group_sum_kernel(int64_t nvec_out, int G, int R, int dv, const T* __restrict__ in,
                                                        T* __restrict__ out) {
  constexpr int VEC = LV<T>::VEC;
  using P = LPack<T, VEC>;
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

static bool dt_ok(int dt) { return dt == VCT_F32 || dt == VCT_BF16; }
static int vec_of(int dt) { return dt == VCT_BF16 ? 8 : 4; }

// what the three entries pass on; a member its kind does not use stays 0 / NULL
struct LossArgs {
  int dtype, N, S, V;
  const void* logits;
  int64_t ldl;
  const int64_t* labels;
  int64_t lbstride, pad_id;
  float alpha, eps;
  const float* seq_w;
  float *loss, *stats, *tok_logp;
  void* dlogits;
  int64_t ld_dl;
  float* row_ws;
  void* stream;
};

template <int KIND> static int caption_loss(const LossArgs& p) {
  if (!dt_ok(p.dtype) || !p.logits || !p.labels || !p.loss || !p.row_ws) return VCT_E_ARG;
  if (p.N <= 0 || p.S <= 0 || p.V <= 0 || p.N % p.S) return VCT_E_SHAPE;
  const int vec = vec_of(p.dtype);
  const int64_t vround = ((int64_t)p.V + vec - 1) / vec * vec;
  if (p.ldl < vround || p.ldl % vec || ((uintptr_t)p.logits & 15)) return VCT_E_ALIGN;       // rows are read as 16-byte vectors
  if (p.dlogits && (p.ld_dl < vround || p.ld_dl % vec || ((uintptr_t)p.dlogits & 15))) return VCT_E_ALIGN;
  if ((p.dlogits && p.ld_dl > (int64_t)8 * 1024 * vec) || vround > (int64_t)8 * 1024 * vec) return VCT_E_SHAPE;   // row must fit the register tile
  hipStream_t st = (hipStream_t)p.stream;
  const int N = p.N;
  vct::launch(count_valid_kernel, dim3(1), dim3(1024), 0, st, N, p.S, p.labels, p.lbstride, p.pad_id, p.row_ws + 2 * (size_t)N);
  VCT_CHECK_LAUNCH();
  const int64_t width = p.dlogits ? (p.ld_dl > vround ? p.ld_dl : vround) : vround;
  const bool small = width <= (int64_t)4 * 1024 * vec;
#define VCT_ROWS(T_, IT_, NT_) vct::launch((sce_loss_kernel<T_, IT_, NT_, KIND>), dim3(N), dim3(NT_), 0, st, N, p.S, p.V, (const T_*)p.logits, \
                                           p.ldl, p.labels, p.lbstride, p.pad_id, p.alpha, p.seq_w, p.tok_logp, (T_*)p.dlogits, p.ld_dl,   \
                                           p.row_ws, p.eps)
  // bf16, rows up to 4096 vectors: 512 threads x 8 vectors (4 workgroups per CU) -- measured in the step at V = 30522: 114 us against
  // 136 us for 1024 x 4 and 126 us for 256 x 16 (5.2 TB/s of HBM traffic)
  if (p.dtype == VCT_BF16) { if (small) VCT_ROWS(bf16_t, 8, 512); else VCT_ROWS(bf16_t, 8, 1024); }
  else { if (small) VCT_ROWS(float, 4, 1024); else VCT_ROWS(float, 8, 1024); }
#undef VCT_ROWS
  VCT_CHECK_LAUNCH();
  vct::launch(sce_finalize_kernel<KIND>, dim3(1), dim3(1024), 0, st, N, p.alpha, (const float*)p.row_ws, p.loss, p.stats);
  VCT_CHECK_LAUNCH();
  return VCT_OK;
}

extern "C" int vct_sce_loss(int dtype, int N, int S, int V, const void* logits, int64_t ldl, const int64_t* labels,
                            int64_t label_batch_stride, int64_t pad_id, float alpha, float* loss_out, void* dlogits,
                            int64_t ld_dl, float* row_ws, void* stream) {
  return caption_loss<SCE>({dtype, N, S, V, logits, ldl, labels, label_batch_stride, pad_id, alpha, 0.0f, nullptr, loss_out, nullptr,
                            nullptr, dlogits, ld_dl, row_ws, stream});
}

extern "C" int vct_sce_loss_ls(int dtype, int N, int S, int V, const void* logits, int64_t ldl, const int64_t* labels,
                               int64_t label_batch_stride, int64_t pad_id, float alpha, float smoothing, float* loss_out,
                               float* stats_out, void* dlogits, int64_t ld_dl, float* row_ws, void* stream) {
  if (!(smoothing >= 0.0f && smoothing < 1.0f)) return VCT_E_ARG;       // NaN fails both comparisons
  return caption_loss<LS>({dtype, N, S, V, logits, ldl, labels, label_batch_stride, pad_id, alpha, smoothing, nullptr, loss_out,
                           stats_out, nullptr, dlogits, ld_dl, row_ws, stream});
}

extern "C" int vct_wce_loss(int dtype, int N, int S, int V, const void* logits, int64_t ldl, const int64_t* labels,
                            int64_t label_batch_stride, int64_t pad_id, const float* seq_w, float* loss_out, float* tok_logp,
                            void* dlogits, int64_t ld_dl, float* row_ws, void* stream) {
  return caption_loss<WCE>({dtype, N, S, V, logits, ldl, labels, label_batch_stride, pad_id, 1.0f, 0.0f, seq_w, loss_out, nullptr,
                            tok_logp, dlogits, ld_dl, row_ws, stream});
}

extern "C" int vct_group_sum(int dtype, int B, int G, int R, int d, const void* in, void* out, void* stream) {
  if (!dt_ok(dtype) || !in || !out) return VCT_E_ARG;
  const int vec = vec_of(dtype);
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
