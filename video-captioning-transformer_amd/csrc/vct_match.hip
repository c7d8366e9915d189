// The video-text matching head on gfx950 (include/vct_hip.h: vct_match_loss, vct_match_agg_*, vct_scale).
//
// replaces: ClipSymmetricalLoss / ClipSymmetricalLoss_WithDualSoftmax (model/loss.py:7-67 of the reference) with their autograd
// backward down to the un-normalised video feature, the `memory[:, 0]` slice that feeds Matching (MMEncoder.py: agg_feat) with the
// backward of that slice, and the `loss_beta * cap_loss + (1 - loss_beta) * match_loss` mix of the two tasks' gradients
// (MMT4Caption.py:133-147).
//
// vct_match_loss, everything fp32, sim[i, j] = t^_i . v^_j (text rows i, video columns j):
//   1 match_sim_kernel    16 x 16 tiles of the raw products over LDS K-chunks of 64 (a k-ordered fmaf chain per element), the row
//                         norms summed in a fixed order by every tile that needs them; S = raw / (|t_i| |v_j|)
//   2 match_colz_kernel   CSL_WDS only: per column j the max and the sum of exp of S[:, j] / tau (the softmax over the text index)
//   3 match_stats_kernel  2 B workgroups: log-sum-exp of every row and of every column of the logits; writes `sim` when asked
//   4 match_grad_kernel   four columns j per workgroup: dS[:, j] (CSL_WDS: through the column softmax, in a cancellation-free form) into LDS,
//                         dv^_j = sum_i dS[i, j] t^_i in i order, back through the normalisation; one dtemp partial per workgroup
//   5 match_final_kernel  one workgroup: the loss and dtemp from the per-row / per-workgroup partials, in index order
// Forward only (dvid == NULL) skips 4.  Every reduction is wave shuffles (a butterfly: the same tree on every call), then LDS, then
// a serial pass in index order; there is no floating-point atomic, so two calls on the same inputs agree bitwise.
#include "vct_common.h"
#include <math.h>

namespace vct {

constexpr int MT_THREADS = 256;
constexpr int MT_NW = MT_THREADS / WAVE;
constexpr int MT_MAX_B = 256;       // one row (or column) element per thread of a workgroup
constexpr int MT_MAX_D = 1024;      // one 16-byte vector of a feature row per thread
constexpr int MT_TILE = 16;
constexpr int MT_KC = 64;
constexpr int MT_JB = 4;            // columns per workgroup of the gradient kernel

struct MatchWs {
  float* S;        // [B, B]
  float* rt;       // [B] 1 / |t_i|
  float* rv;       // [B] 1 / |v_j|
  float* rlse;     // [B]
  float* clse;     // [B]
  float* cmz;      // [B] CSL_WDS: max_i S[i, j] / tau
  float* csz;      // [B] CSL_WDS: sum_i exp(S[i, j] / tau - cmz[j])
  float* part;     // [(B + MT_JB - 1) / MT_JB] dtemp partials
};

__host__ __device__ inline long long match_ws_floats(int B) { return (long long)B * B + 6LL * B + MT_MAX_B / MT_JB; }

__host__ __device__ inline MatchWs match_ws(float* base, int B) {
  MatchWs w;
  w.S = base;
  w.rt = base + (size_t)B * B;
  w.rv = w.rt + B;
  w.rlse = w.rv + B;
  w.clse = w.rlse + B;
  w.cmz = w.clse + B;
  w.csz = w.cmz + B;
  w.part = w.csz + B;
  return w;
}

// the logit the two cross-entropies see at (i, j): S * exp(temp) or S (CSL), S * softmax_i(S / tau) * B (CSL_WDS); p = that softmax
__device__ __forceinline__ float match_logit(const MatchWs& w, int B, int kind, float scale, float inv_tau, int i, int j, float& s, float& p) {
  s = w.S[(size_t)i * B + j];
  if (kind == VCT_MATCH_CSL) { p = 0.0f; return s * scale; }
  p = expf(s * inv_tau - w.cmz[j]) / w.csz[j];
  return (s * p) * (float)B;
}

__global__ __launch_bounds__(MT_THREADS) void match_sim_kernel(const float* __restrict__ text, long long ldt, const float* __restrict__ vid,
                                                               long long ldv, int B, int Dt, MatchWs w) {
  __shared__ float ta[MT_TILE][MT_KC + 1], tb[MT_TILE][MT_KC + 1];
  __shared__ float ssa[MT_TILE][MT_TILE], ssb[MT_TILE][MT_TILE];
  const int r = threadIdx.x >> 4, c4 = threadIdx.x & 15;      // loader: row r of the tile, vector c4 of the K chunk; product: (ty, tx)
  const int i0 = blockIdx.y * MT_TILE, j0 = blockIdx.x * MT_TILE;
  float acc = 0.0f, sa = 0.0f, sb = 0.0f;
  for (int k0 = 0; k0 < Dt; k0 += MT_KC) {
    const int k = k0 + 4 * c4;
    float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = a;
    if (k < Dt) {                                             // (Dt is a multiple of 4: a vector is inside the row or outside it)
      if (i0 + r < B) a = *reinterpret_cast<const float4*>(text + (size_t)(i0 + r) * ldt + k);
      if (j0 + r < B) b = *reinterpret_cast<const float4*>(vid + (size_t)(j0 + r) * ldv + k);
    }
    sa = fmaf(a.x, a.x, sa); sa = fmaf(a.y, a.y, sa); sa = fmaf(a.z, a.z, sa); sa = fmaf(a.w, a.w, sa);
    sb = fmaf(b.x, b.x, sb); sb = fmaf(b.y, b.y, sb); sb = fmaf(b.z, b.z, sb); sb = fmaf(b.w, b.w, sb);
    ta[r][4 * c4 + 0] = a.x; ta[r][4 * c4 + 1] = a.y; ta[r][4 * c4 + 2] = a.z; ta[r][4 * c4 + 3] = a.w;
    tb[r][4 * c4 + 0] = b.x; tb[r][4 * c4 + 1] = b.y; tb[r][4 * c4 + 2] = b.z; tb[r][4 * c4 + 3] = b.w;
    __syncthreads();
#pragma unroll 16
    for (int kk = 0; kk < MT_KC; kk++) acc = fmaf(ta[r][kk], tb[c4][kk], acc);
    __syncthreads();
  }
  ssa[r][c4] = sa;
  ssb[r][c4] = sb;
  __syncthreads();
  float na = 0.0f, nb = 0.0f;
#pragma unroll
  for (int q = 0; q < MT_TILE; q++) { na += ssa[r][q]; nb += ssb[c4][q]; }
  const float ra = 1.0f / sqrtf(na), rb = 1.0f / sqrtf(nb);
  const int i = i0 + r, j = j0 + c4;
  if (i < B && j < B) w.S[(size_t)i * B + j] = (acc * ra) * rb;
  if (blockIdx.x == 0 && c4 == 0 && i < B) w.rt[i] = ra;
  if (blockIdx.y == 0 && r == 0 && j < B) w.rv[j] = rb;
}

__global__ __launch_bounds__(MT_THREADS) void match_colz_kernel(int B, const float* __restrict__ temp, MatchWs w) {
  __shared__ float red[MT_NW];
  const int j = blockIdx.x, i = threadIdx.x;
  const float inv_tau = 1.0f / temp[0];
  const float z = i < B ? w.S[(size_t)i * B + j] * inv_tau : -INFINITY;
  const float m = block_max<MT_NW>(z, red);
  const float s = block_sum<MT_NW>(i < B ? expf(z - m) : 0.0f, red);
  if (i == 0) { w.cmz[j] = m; w.csz[j] = s; }
}

__global__ __launch_bounds__(MT_THREADS) void match_stats_kernel(int B, int kind, int tkind, const float* __restrict__ temp, MatchWs w,
                                                                 float* __restrict__ sim, long long ld_sim) {
  __shared__ float red[MT_NW];
  const bool row = (int)blockIdx.x < B;
  const int fixed = row ? blockIdx.x : blockIdx.x - B, t = threadIdx.x;
  const int i = row ? fixed : t, j = row ? t : fixed;
  const float scale = tkind == VCT_MATCH_TEMP_EXP ? expf(temp[0]) : 1.0f;
  const float inv_tau = tkind == VCT_MATCH_TEMP_DIV ? 1.0f / temp[0] : 0.0f;
  float l = -INFINITY, s, p;
  if (t < B) l = match_logit(w, B, kind, scale, inv_tau, i, j, s, p);
  const float m = block_max<MT_NW>(l, red);
  const float se = block_sum<MT_NW>(t < B ? expf(l - m) : 0.0f, red);
  if (t == 0) (row ? w.rlse : w.clse)[fixed] = m + logf(se);
  if (row && sim != nullptr && t < B) sim[(size_t)i * ld_sim + j] = l;
}

__global__ __launch_bounds__(MT_THREADS) void match_grad_kernel(const float* __restrict__ text, long long ldt, const float* __restrict__ vid,
                                                                long long ldv, int B, int Dt, int kind, int tkind,
                                                                const float* __restrict__ temp, MatchWs w, float* __restrict__ dvid,
                                                                long long ld_dv) {
  __shared__ float red[MT_NW];
  __shared__ float ds[MT_JB][MT_MAX_B];
  __shared__ float rts[MT_MAX_B];
  __shared__ float pcol[MT_MAX_B], hcol[MT_MAX_B];
  const int t = threadIdx.x, j0 = blockIdx.x * MT_JB;
  const float scale = tkind == VCT_MATCH_TEMP_EXP ? expf(temp[0]) : 1.0f;
  const float inv_tau = tkind == VCT_MATCH_TEMP_DIV ? 1.0f / temp[0] : 0.0f;
  const float inv_2b = 0.5f / (float)B;
  // ---- dS[:, j0 .. j0 + 3] (thread t = row i) and this workgroup's share of d(temperature) ----
  float tsum = 0.0f;
  const float rl = t < B ? w.rlse[t] : 0.0f;
  rts[t] = t < B ? w.rt[t] : 0.0f;
#pragma unroll
  for (int jj = 0; jj < MT_JB; jj++) {
    const int j = j0 + jj;                                    // (uniform over the workgroup)
    float g = 0.0f, l = 0.0f, s = 0.0f, p = 0.0f;
    if (t < B && j < B) {
      l = match_logit(w, B, kind, scale, inv_tau, t, j, s, p);
      g = ((expf(l - rl) + expf(l - w.clse[j])) - (t == j ? 2.0f : 0.0f)) * inv_2b;
    }
    float d;
    if (kind == VCT_MATCH_CSL) {
      d = g * scale;
      tsum += g * l;                                          // d(logit) / d(temp) = logit for S * exp(temp)
    } else {
      // softmax backward over the column: dZ[i] = P[i] (H[i] - sum_k P[k] H[k]).  With a small tau one P[i] is close to 1 and that
      // difference cancels to (1 - P[i]) of its operands; sum_k P[k] (H[i] - H[k]) is the same number (sum_k P[k] = 1) without it.
      const float h = (g * (float)B) * s;                     // dLoss / dP[i, j]
      __syncthreads();                                        // (the previous column's readers are done)
      pcol[t] = p;
      hcol[t] = h;
      __syncthreads();
      float e = 0.0f;
      for (int k = 0; k < B; k++) e = fmaf(pcol[k], h - hcol[k], e);
      const float dz = p * e;                                 // dLoss / d(S / tau)[i, j]
      d = (g * (float)B) * p + dz * inv_tau;
      tsum -= (dz * s) * (inv_tau * inv_tau);
    }
    ds[jj][t] = d;
  }
  const float part = block_sum<MT_NW>(tsum, red);             // (also the barrier that publishes ds / rts)
  if (t == 0) w.part[blockIdx.x] = part;
  // ---- dv^_j = sum_i dS[i, j] t^_i: thread t owns the 16-byte vector t of the feature row ----
  const bool on = 4 * t < Dt;
  float4 acc[MT_JB];
#pragma unroll
  for (int jj = 0; jj < MT_JB; jj++) acc[jj] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (on) {
    const float* tp = text + 4 * t;
    for (int i = 0; i < B; i++) {
      float4 x = *reinterpret_cast<const float4*>(tp + (size_t)i * ldt);
      const float r = rts[i];
      x.x *= r; x.y *= r; x.z *= r; x.w *= r;
#pragma unroll
      for (int jj = 0; jj < MT_JB; jj++) {
        const float d = ds[jj][i];
        acc[jj].x = fmaf(d, x.x, acc[jj].x); acc[jj].y = fmaf(d, x.y, acc[jj].y);
        acc[jj].z = fmaf(d, x.z, acc[jj].z); acc[jj].w = fmaf(d, x.w, acc[jj].w);
      }
    }
  }
  // ---- back through v^ = v / |v|: dv = (dv^ - v^ (v^ . dv^)) / |v| ----
#pragma unroll
  for (int jj = 0; jj < MT_JB; jj++) {
    const int j = j0 + jj;
    if (j >= B) break;                                        // (uniform)
    const float rv = w.rv[j];
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (on) {
      v = *reinterpret_cast<const float4*>(vid + (size_t)j * ldv + 4 * t);
      v.x *= rv; v.y *= rv; v.z *= rv; v.w *= rv;
    }
    const float4 a = acc[jj];
    const float dot = block_sum<MT_NW>(fmaf(v.w, a.w, fmaf(v.z, a.z, fmaf(v.y, a.y, v.x * a.x))), red);
    if (on) {
      float4 o;
      o.x = (a.x - v.x * dot) * rv; o.y = (a.y - v.y * dot) * rv; o.z = (a.z - v.z * dot) * rv; o.w = (a.w - v.w * dot) * rv;
      *reinterpret_cast<float4*>(dvid + (size_t)j * ld_dv + 4 * t) = o;
    }
  }
}

__global__ __launch_bounds__(MT_THREADS) void match_final_kernel(int B, int kind, int tkind, const float* __restrict__ temp, MatchWs w,
                                                                 float* __restrict__ loss, float* __restrict__ dtemp, int nparts) {
  __shared__ float red[MT_NW];
  const int t = threadIdx.x;
  const float scale = tkind == VCT_MATCH_TEMP_EXP ? expf(temp[0]) : 1.0f;
  const float inv_tau = tkind == VCT_MATCH_TEMP_DIV ? 1.0f / temp[0] : 0.0f;
  float term = 0.0f;
  if (t < B) {
    float s, p;
    const float l = match_logit(w, B, kind, scale, inv_tau, t, t, s, p);
    term = (w.rlse[t] - l) + (w.clse[t] - l);
  }
  const float total = block_sum<MT_NW>(term, red);
  if (t == 0) loss[0] = total * (0.5f / (float)B);
  if (dtemp != nullptr) {                                     // (uniform)
    const float d = block_sum<MT_NW>(t < nparts ? w.part[t] : 0.0f, red);
    if (t == 0) dtemp[0] = d;
  }
}

// ---- the aggregation row of every sample <-> the head's fp32 [B, d] ---------------------------------------------------------------
template <typename T, int VEC> struct alignas(sizeof(T) * VEC) MPack { T v[VEC]; };

template <typename T>
__global__ __launch_bounds__(MT_THREADS) void match_agg_fwd_kernel(const T* __restrict__ mem, float* __restrict__ agg, int Te, int nvec,
                                                                   long long total) {
  constexpr int VEC = 16 / sizeof(T);
  const long long it = (long long)blockIdx.x * MT_THREADS + threadIdx.x;
  if (it >= total) return;
  const long long b = it / nvec;
  const int c = (int)(it % nvec) * VEC;
  const MPack<T, VEC> x = *reinterpret_cast<const MPack<T, VEC>*>(mem + ((size_t)b * Te * nvec) * VEC + c);
  float* o = agg + (size_t)b * nvec * VEC + c;
#pragma unroll
  for (int q = 0; q < VEC; q += 4)
    *reinterpret_cast<float4*>(o + q) = make_float4(to_f<T>(x.v[q]), to_f<T>(x.v[q + 1]), to_f<T>(x.v[q + 2]), to_f<T>(x.v[q + 3]));
}

// A product that stays a product: hipcc contracts a * b + c into one fma (its __fmul_rn / __fadd_rn are plain operators, and a
// contract(off) pragma does not reach the backend's fusion); a value that went through an (empty) asm statement cannot be fused.
__device__ __forceinline__ float rounded_mul(float a, float b) {
  float v = a * b;
  asm volatile("" : "+v"(v));
  return v;
}

// dmem[b * Te + r] = beta * dmem[b * Te + r] + (r == 0 ? (1 - beta) * dagg[b] : 0); empty: the old contents are not read.  Separately
// rounded products and one add (no contraction), then one rounding to T: the arithmetic a test can restate exactly.
template <typename T>
__global__ __launch_bounds__(MT_THREADS) void match_agg_bwd_kernel(T* __restrict__ dmem, const float* __restrict__ dagg, int Te, int nvec,
                                                                   long long total, float beta, int empty) {
  constexpr int VEC = 16 / sizeof(T);
  using P = MPack<T, VEC>;
  const long long it = (long long)blockIdx.x * MT_THREADS + threadIdx.x;
  if (it >= total) return;
  const long long row = it / nvec;
  const int c = (int)(it % nvec) * VEC;
  const long long b = row / Te;
  const bool first = row % Te == 0;
  const float omb = 1.0f - beta;
  P* at = reinterpret_cast<P*>(dmem + (size_t)it * VEC);
  P o;
  if (!empty) o = *at;
#pragma unroll
  for (int q = 0; q < VEC; q++) {
    float y = empty ? 0.0f : rounded_mul(beta, to_f<T>(o.v[q]));
    if (first) y += rounded_mul(omb, dagg[(size_t)b * nvec * VEC + c + q]);
    o.v[q] = from_f<T>(y);
  }
  *at = o;
}

__global__ __launch_bounds__(MT_THREADS) void scale_kernel(float* __restrict__ x, long long n, float s) {
  const long long it = (long long)blockIdx.x * MT_THREADS + threadIdx.x;
  const long long at = it * 4;
  if (at + 4 <= n) {
    float4 v = *reinterpret_cast<float4*>(x + at);
    v.x *= s; v.y *= s; v.z *= s; v.w *= s;
    *reinterpret_cast<float4*>(x + at) = v;
  } else {
    for (long long k = at; k < n; k++) x[k] *= s;
  }
}

// out = a * x + b * y (y may be NULL: out = a * x); separately rounded products, one add
__global__ __launch_bounds__(MT_THREADS) void axpby_kernel(float* __restrict__ out, const float* __restrict__ x, float a,
                                                           const float* __restrict__ y, float b, long long n) {
  const long long i = (long long)blockIdx.x * MT_THREADS + threadIdx.x;
  if (i >= n) return;
  const float ax = rounded_mul(a, x[i]);
  out[i] = y != nullptr ? ax + rounded_mul(b, y[i]) : ax;
}

}  // namespace vct
using namespace vct;

static bool mt_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }

extern "C" int64_t vct_match_loss_workspace_bytes(int B, int Dt) {
  if (B < 1 || B > MT_MAX_B || Dt < 4 || Dt > MT_MAX_D || Dt % 4) return 0;
  return (int64_t)(match_ws_floats(B) * 4);
}

extern "C" int vct_match_loss(const vct_match_loss_desc* p, void* stream) {
  if (p == nullptr) return VCT_E_ARG;
  if (p->loss_kind != VCT_MATCH_CSL && p->loss_kind != VCT_MATCH_CSL_WDS) return VCT_E_ARG;
  if (p->temp_kind != VCT_MATCH_TEMP_NONE && p->temp_kind != VCT_MATCH_TEMP_EXP && p->temp_kind != VCT_MATCH_TEMP_DIV) return VCT_E_ARG;
  // CSL multiplies by exp(temp) or has none; CSL_WDS divides by tau and is not defined without one
  if (p->loss_kind == VCT_MATCH_CSL ? p->temp_kind == VCT_MATCH_TEMP_DIV : p->temp_kind != VCT_MATCH_TEMP_DIV) return VCT_E_ARG;
  if ((p->temp_kind != VCT_MATCH_TEMP_NONE) != (p->temp != nullptr)) return VCT_E_ARG;
  if (!p->text || !p->vid || !p->loss || !p->workspace) return VCT_E_ARG;
  if (p->B < 1 || p->B > MT_MAX_B || p->Dt < 4 || p->Dt > MT_MAX_D || p->Dt % 4) return VCT_E_SHAPE;
  if (p->ld_text < p->Dt || p->ld_vid < p->Dt || (p->dvid && p->ld_dvid < p->Dt) || (p->sim && p->ld_sim < p->B)) return VCT_E_SHAPE;
  if (p->ld_text % 4 || p->ld_vid % 4 || (p->dvid && p->ld_dvid % 4)) return VCT_E_ALIGN;
  if (!mt_aligned(p->text) || !mt_aligned(p->vid) || !mt_aligned(p->dvid) || !mt_aligned(p->workspace)) return VCT_E_ALIGN;
  if (p->workspace_bytes < vct_match_loss_workspace_bytes(p->B, p->Dt)) return VCT_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int B = p->B, Dt = p->Dt, kind = p->loss_kind, tkind = p->temp_kind;
  const MatchWs w = match_ws((float*)p->workspace, B);
  const long long ldt = p->ld_text, ldv = p->ld_vid, ld_dv = p->ld_dvid, ld_sim = p->ld_sim;
  const unsigned tiles = (unsigned)((B + MT_TILE - 1) / MT_TILE);
  vct::launch(match_sim_kernel, dim3(tiles, tiles), dim3(MT_THREADS), 0, st, p->text, ldt, p->vid, ldv, B, Dt, w);
  VCT_CHECK_LAUNCH();
  if (kind == VCT_MATCH_CSL_WDS) {
    vct::launch(match_colz_kernel, dim3((unsigned)B), dim3(MT_THREADS), 0, st, B, p->temp, w);
    VCT_CHECK_LAUNCH();
  }
  vct::launch(match_stats_kernel, dim3((unsigned)(2 * B)), dim3(MT_THREADS), 0, st, B, kind, tkind, p->temp, w, p->sim, ld_sim);
  VCT_CHECK_LAUNCH();
  const int nparts = (B + MT_JB - 1) / MT_JB;
  if (p->dvid != nullptr) {
    vct::launch(match_grad_kernel, dim3((unsigned)nparts), dim3(MT_THREADS), 0, st, p->text, ldt, p->vid, ldv, B, Dt, kind, tkind, p->temp, w,
                p->dvid, ld_dv);
    VCT_CHECK_LAUNCH();
  }
  vct::launch(match_final_kernel, dim3(1), dim3(MT_THREADS), 0, st, B, kind, tkind, p->temp, w, p->loss,
              (p->temp != nullptr && p->dvid != nullptr) ? p->dtemp : (float*)nullptr, nparts);
  VCT_CHECK_LAUNCH();
  return VCT_OK;
}

static int agg_prepare(const vct_match_agg_desc* p, int& nvec) {
  if (p == nullptr) return VCT_E_ARG;
  if (p->dtype != VCT_F32 && p->dtype != VCT_BF16) return VCT_E_ARG;
  if (p->B < 1 || p->Te < 1 || p->d < 1) return VCT_E_SHAPE;
  const int vec = p->dtype == VCT_BF16 ? 8 : 4;
  if (p->d % vec) return VCT_E_ALIGN;
  nvec = p->d / vec;
  if (((long long)p->B * p->Te * nvec + MT_THREADS - 1) / MT_THREADS > 0x7fffffffLL) return VCT_E_SHAPE;
  return VCT_OK;
}

extern "C" int vct_match_agg_fwd(const vct_match_agg_desc* p, void* stream) {
  int nvec;
  const int rc = agg_prepare(p, nvec);
  if (rc != VCT_OK) return rc;
  if (!p->mem || !p->agg) return VCT_E_ARG;
  if (!mt_aligned(p->mem) || !mt_aligned(p->agg)) return VCT_E_ALIGN;
  const long long total = (long long)p->B * nvec;
  const dim3 grid((unsigned)((total + MT_THREADS - 1) / MT_THREADS));
  hipStream_t st = (hipStream_t)stream;
  if (p->dtype == VCT_BF16)
    vct::launch((match_agg_fwd_kernel<bf16_t>), grid, dim3(MT_THREADS), 0, st, (const bf16_t*)p->mem, p->agg, p->Te, nvec, total);
  else
    vct::launch((match_agg_fwd_kernel<float>), grid, dim3(MT_THREADS), 0, st, (const float*)p->mem, p->agg, p->Te, nvec, total);
  VCT_CHECK_LAUNCH();
  return VCT_OK;
}

extern "C" int vct_match_agg_bwd(const vct_match_agg_desc* p, void* stream) {
  int nvec;
  const int rc = agg_prepare(p, nvec);
  if (rc != VCT_OK) return rc;
  if (!p->dmem || !p->dagg) return VCT_E_ARG;
  if (!(p->beta >= 0.0f && p->beta <= 1.0f)) return VCT_E_ARG;
  if (!mt_aligned(p->dmem) || !mt_aligned(p->dagg)) return VCT_E_ALIGN;
  const long long total = (long long)p->B * p->Te * nvec;
  const dim3 grid((unsigned)((total + MT_THREADS - 1) / MT_THREADS));
  hipStream_t st = (hipStream_t)stream;
  const int empty = p->empty != 0;
  if (p->dtype == VCT_BF16)
    vct::launch((match_agg_bwd_kernel<bf16_t>), grid, dim3(MT_THREADS), 0, st, (bf16_t*)p->dmem, p->dagg, p->Te, nvec, total, p->beta, empty);
  else
    vct::launch((match_agg_bwd_kernel<float>), grid, dim3(MT_THREADS), 0, st, (float*)p->dmem, p->dagg, p->Te, nvec, total, p->beta, empty);
  VCT_CHECK_LAUNCH();
  return VCT_OK;
}

extern "C" int vct_scale(float* x, int64_t n, float s, void* stream) {
  if (x == nullptr) return VCT_E_ARG;
  if (n < 0) return VCT_E_SHAPE;
  if (!mt_aligned(x)) return VCT_E_ALIGN;
  if (n == 0) return VCT_OK;
  const long long blocks = ((long long)n + 4LL * MT_THREADS - 1) / (4LL * MT_THREADS);
  if (blocks > 0x7fffffffLL) return VCT_E_SHAPE;
  vct::launch(scale_kernel, dim3((unsigned)blocks), dim3(MT_THREADS), 0, (hipStream_t)stream, x, (long long)n, s);
  VCT_CHECK_LAUNCH();
  return VCT_OK;
}

extern "C" int vct_axpby(float* out, const float* x, float a, const float* y, float b, int64_t n, void* stream) {
  if (out == nullptr || x == nullptr) return VCT_E_ARG;
  if (n < 0) return VCT_E_SHAPE;
  if (n == 0) return VCT_OK;
  const long long blocks = ((long long)n + MT_THREADS - 1) / MT_THREADS;
  if (blocks > 0x7fffffffLL) return VCT_E_SHAPE;
  vct::launch(axpby_kernel, dim3((unsigned)blocks), dim3(MT_THREADS), 0, (hipStream_t)stream, out, x, a, y, b, (long long)n);
  VCT_CHECK_LAUNCH();
  return VCT_OK;
}
