// Encoder front end with every option of the reference's `mme` block on gfx950: the n >= 1 feature streams' unify outputs -> the
// stack input and its key padding, and the backward of that (include/vct_hip.h, vct_enc_frontend_ex_*).  A generalisation of
// vct_mm_frontend.hip (same row layout, vector widths and fixed-order reductions); the shipped combination ('avg', 'encoding', no
// norm) keeps its own kernels.
//
// replaces: GlobalAggregation('avg' | 'max') + cat + TemporalEncoding | TemporalEmbedding + ModalEmbedding + the `temp + modal + feats`
// add + Dropout(LayerNorm(.)) (do_norm) of the reference's MultiModalEncoder.forward (model/MMEncoder.py:12-48, 83-104, 118-160,
// 173-197, 240-276), the mask cat (:252-266), and their autograd backward.
//
// fwd, one launch, grid (B, n), 4 waves: workgroup (b, i) owns stream i's T_i + 1 rows of sample b, ONE WAVE PER ROW with the row in
// registers (<= 16 values per lane => d <= 1024, as csrc/vct_norm.hip):
//   pre(agg row) = (temporal + modal) + mean_t | max_t u_i[b, t]     (fp32, all T_i rows in row order, pads included)
//   pre(row t)   = (temporal + modal) + u_i[b, t]
//   x0 = pre, or dropout(LayerNorm(pre)) with the row statistics by wave shuffles (two-pass variance), mean / rstd stored.
// bwd, row workgroups (b, i) in front:
//   norm: per row, pre recomputed in fp32 from u, dpre = LayerNorm backward of dx x mask; dpre goes to memory in fp32, the workgroup's
//         dgamma / dbeta column partials (rows in wave order, waves in order) to param_ws[b*n + i]
//   max:  the wave of the aggregation row records, per column, the first row that holds the maximum
//   du_i[b, t] = dpre[b, off_i+1+t] + dpre[b, off_i] / T_i   |   + dpre[b, off_i] where t is that first maximal row
// and behind them (same launch without the norm; a second launch with it, because they read every sample's dpre):
//   (label l, column group g):  d_modal[l, g's columns] as vct_mm_frontend_bwd
//   (memory row s, column group g): when s is the first row that reads its embedding row e, d_emb[e, g's columns] = sum over the
//                   (b, s') with tidx[s'] == e of dpre[b, s']; a few more workgroups zero the rows nobody reads
// both as "64 row lanes each sum a fixed residue class in order, then the lane partials in lane order".  No atomics anywhere.
#include "vct_common.h"

namespace vct {

constexpr int FX_THREADS = 256;
constexpr int FX_WAVES = FX_THREADS / WAVE;
constexpr int FX_CV = 4;                          // 16-byte column vectors per reduction pass
constexpr int FX_LANES = FX_THREADS / FX_CV;      // row lanes per reduction pass
constexpr int FX_MAX_ROWS = 1024;                 // S limit (the per-key row list lives in LDS)
constexpr int FX_MAX_D = 1024;                    // a row lives in one wave's registers
constexpr int FX_ZERO_WGS = 8;                    // workgroups that zero the unread rows of d_emb

template <typename T> struct FxCfg;
template <> struct FxCfg<float> { static constexpr int VEC = 4, MAXIT = 4; };
template <> struct FxCfg<bf16_t> { static constexpr int VEC = 8, MAXIT = 2; };
template <typename T, int VEC> struct alignas(16) FxPack { T v[VEC]; };

struct FxArgs {
  int n, B, d, S, n_labels, agg, learned, norm, emb_rows;
  uint32_t site; float p_drop;
  int T[VCT_MM_MAX_MODAL];
  int off[VCT_MM_MAX_MODAL];
  const void* u[VCT_MM_MAX_MODAL];
  const uint8_t* mask[VCT_MM_MAX_MODAL];
  void* du[VCT_MM_MAX_MODAL];
  const float* temp; const float* emb_w; const int32_t* tidx; const float* modal_w; const int32_t* labels;
  const float* gamma; const float* beta; const uint32_t* seed;
  void* x0; uint8_t* key_pad; float* mean; float* rstd;
  const void* dx; float* d_modal; float* d_emb; float* dpre; float* param_ws;
};

// temporal row + modal-embedding row (fp32, 4 columns from c): what the reference adds to the features
__device__ __forceinline__ float4 fx_row_add(const FxArgs& a, int row, int c) {
  float4 tp;
  if (a.learned) {
    const int e = a.tidx[row];
    tp = (unsigned)e < (unsigned)a.emb_rows ? *reinterpret_cast<const float4*>(a.emb_w + (size_t)e * a.d + c)
                                            : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  } else {
    tp = *reinterpret_cast<const float4*>(a.temp + (size_t)row * a.d + c);
  }
  if (a.n < 2) return tp;
  const int l = a.labels[row];
  if ((unsigned)l >= (unsigned)a.n_labels) return tp;
  const float4 md = *reinterpret_cast<const float4*>(a.modal_w + (size_t)l * a.d + c);
  return make_float4(tp.x + md.x, tp.y + md.y, tp.z + md.z, tp.w + md.w);
}

// One wave: pre of row r of a stream (r = 0: the aggregation row, else frame r - 1) of one sample, fp32, into v (zeros past the row's
// end); u = the sample's [Tn, d] unify output, srow = the row's index in [0, S).  am: per column of the aggregation row under 'max',
// the first frame that holds the maximum.  ADD = false: the aggregate alone (the backward's argmax scan without the norm: temp / emb_w /
// modal_w are not read, and need not exist).
template <typename T, bool ADD = true>
__device__ __forceinline__ void fx_pre_row(const FxArgs& a, const T* __restrict__ u, int Tn, int srow, int r, int lane,
                                           float (&v)[FxCfg<T>::MAXIT][FxCfg<T>::VEC], int (&am)[FxCfg<T>::MAXIT][FxCfg<T>::VEC]) {
  constexpr int VEC = FxCfg<T>::VEC, MAXIT = FxCfg<T>::MAXIT;
  using P = FxPack<T, VEC>;
  const int d = a.d, nvec = d / VEC;
#pragma unroll
  for (int it = 0; it < MAXIT; it++) {
    const int vi = it * WAVE + lane;
#pragma unroll
    for (int j = 0; j < VEC; j++) { v[it][j] = 0.0f; am[it][j] = 0; }
    if (vi >= nvec) continue;
    float val[VEC];
    if (r > 0) {
      const P uv = *reinterpret_cast<const P*>(u + (size_t)(r - 1) * d + vi * VEC);
#pragma unroll
      for (int j = 0; j < VEC; j++) val[j] = to_f<T>(uv.v[j]);
    } else if (a.agg == VCT_AGG_MAX) {
      const P u0 = *reinterpret_cast<const P*>(u + vi * VEC);
#pragma unroll
      for (int j = 0; j < VEC; j++) val[j] = to_f<T>(u0.v[j]);
      for (int t = 1; t < Tn; t++) {
        const P uv = *reinterpret_cast<const P*>(u + (size_t)t * d + vi * VEC);
#pragma unroll
        for (int j = 0; j < VEC; j++) {
          const float x = to_f<T>(uv.v[j]);
          if (x > val[j]) { val[j] = x; am[it][j] = t; }      // strict: equal maxima stay on the first row
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < VEC; j++) val[j] = 0.0f;
      for (int t = 0; t < Tn; t++) {
        const P uv = *reinterpret_cast<const P*>(u + (size_t)t * d + vi * VEC);
#pragma unroll
        for (int j = 0; j < VEC; j++) val[j] += to_f<T>(uv.v[j]);
      }
#pragma unroll
      for (int j = 0; j < VEC; j++) val[j] = val[j] / (float)Tn;
    }
    if constexpr (ADD) {
#pragma unroll
      for (int q = 0; q < VEC; q += 4) {
        const float4 tm = fx_row_add(a, srow, vi * VEC + q);
        v[it][q + 0] = tm.x + val[q + 0];
        v[it][q + 1] = tm.y + val[q + 1];
        v[it][q + 2] = tm.z + val[q + 2];
        v[it][q + 3] = tm.w + val[q + 3];
      }
    } else {
#pragma unroll
      for (int j = 0; j < VEC; j++) v[it][j] = val[j];
    }
  }
}

template <typename T>
__global__ __launch_bounds__(FX_THREADS) void enc_frontend_ex_fwd_kernel(FxArgs a) {
  constexpr int VEC = FxCfg<T>::VEC, MAXIT = FxCfg<T>::MAXIT;
  using P = FxPack<T, VEC>;
  const int b = blockIdx.x, i = blockIdx.y;
  const int Tn = a.T[i], d = a.d, nvec = d / VEC;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t base = (size_t)b * a.S + a.off[i];
  const T* __restrict__ u = static_cast<const T*>(a.u[i]) + (size_t)b * Tn * d;
  T* __restrict__ x0 = static_cast<T*>(a.x0);
  const Dropout dr = make_dropout(a.norm ? a.seed : nullptr, a.site, a.p_drop);
  for (int r = wave; r <= Tn; r += FX_WAVES) {
    float v[MAXIT][VEC];
    int am[MAXIT][VEC];
    fx_pre_row<T>(a, u, Tn, a.off[i] + r, r, lane, v, am);
    const size_t row = base + r;
    if (a.norm) {
      float sum = 0.0f;
#pragma unroll
      for (int it = 0; it < MAXIT; it++)
#pragma unroll
        for (int j = 0; j < VEC; j++) sum += v[it][j];
      const float mean = wave_sum(sum) / (float)d;
      float sq = 0.0f;
#pragma unroll
      for (int it = 0; it < MAXIT; it++) {
        if (it * WAVE + lane < nvec) {
#pragma unroll
          for (int j = 0; j < VEC; j++) { const float c = v[it][j] - mean; sq += c * c; }
        }
      }
      const float rstd = 1.0f / sqrtf(wave_sum(sq) / (float)d + 1e-5f);
      if (lane == 0) { a.mean[row] = mean; a.rstd[row] = rstd; }
#pragma unroll
      for (int it = 0; it < MAXIT; it++) {
        const int vi = it * WAVE + lane;
        if (vi < nvec) {
          float dm[VEC];
          drop_mults<VEC>(dr, (uint32_t)row * (uint32_t)d + (uint32_t)(vi * VEC), dm);
#pragma unroll
          for (int j = 0; j < VEC; j++) {
            const int c = vi * VEC + j;
            v[it][j] = ((v[it][j] - mean) * rstd * a.gamma[c] + a.beta[c]) * dm[j];
          }
        }
      }
    }
#pragma unroll
    for (int it = 0; it < MAXIT; it++) {
      const int vi = it * WAVE + lane;
      if (vi < nvec) {
        P o;
#pragma unroll
        for (int j = 0; j < VEC; j++) o.v[j] = from_f<T>(v[it][j]);
        *reinterpret_cast<P*>(x0 + row * d + vi * VEC) = o;
      }
    }
  }
  if (a.key_pad != nullptr) {
    const uint8_t* mk = a.mask[i];
    for (int t = threadIdx.x; t <= Tn; t += FX_THREADS)
      a.key_pad[base + t] = (t == 0 || mk == nullptr) ? (uint8_t)0 : (uint8_t)(mk[(size_t)b * Tn + t - 1] != 0);
  }
}

// out[g's columns] = sum over the cnt * B pairs (b, s_rows[k]) of src[b, s]: FX_LANES row lanes each sum a fixed residue class of the
// pairs in order, then the lane partials are summed in lane order.  All threads of the workgroup call it; ends on a barrier.
template <typename T, typename TS>
__device__ __forceinline__ void fx_sum_rows(const FxArgs& a, const TS* __restrict__ src, const int* s_rows, int cnt, int g,
                                            float* __restrict__ out, float* s_red) {
  constexpr int VEC = FxCfg<T>::VEC, W = FX_CV * VEC;
  using P = FxPack<TS, VEC>;
  const int d = a.d, nvec = d / VEC;
  const int cv = threadIdx.x % FX_CV, lane = threadIdx.x / FX_CV;
  const int vi = g * FX_CV + cv;
  float acc[VEC];
#pragma unroll
  for (int j = 0; j < VEC; j++) acc[j] = 0.0f;
  if (vi < nvec && cnt > 0) {
    const int items = a.B * cnt;
    for (int it = lane; it < items; it += FX_LANES) {
      const int b = it / cnt, s = s_rows[it - b * cnt];
      const P v = *reinterpret_cast<const P*>(src + ((size_t)b * a.S + s) * d + vi * VEC);
#pragma unroll
      for (int j = 0; j < VEC; j++) acc[j] += to_f<TS>(v.v[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < VEC; j++) s_red[lane * W + cv * VEC + j] = acc[j];
  __syncthreads();
  if (threadIdx.x < W) {
    const int col = g * W + threadIdx.x;
    if (col < d) {
      float sum = 0.0f;
      for (int r = 0; r < FX_LANES; r++) sum += s_red[r * W + threadIdx.x];
      out[col] = sum;
    }
  }
  __syncthreads();
}

// du of one (sample, stream) from dpre as it sits in memory (TS: the activation type, or fp32 behind the norm's backward)
template <typename T, typename TS>
__device__ __forceinline__ void fx_du_rows(const FxArgs& a, const TS* __restrict__ src, T* __restrict__ du, size_t base, int Tn,
                                           bool by_max, const int* s_arg) {
  constexpr int VEC = FxCfg<T>::VEC;
  using P = FxPack<T, VEC>;
  using PS = FxPack<TS, VEC>;
  const int d = a.d, nvec = d / VEC;
  for (int it = threadIdx.x; it < Tn * nvec; it += FX_THREADS) {
    const int t = it / nvec, vi = it - t * nvec;
    const PS g0 = *reinterpret_cast<const PS*>(src + base * d + vi * VEC);
    const PS g = *reinterpret_cast<const PS*>(src + (base + 1 + t) * d + vi * VEC);
    P o;
#pragma unroll
    for (int j = 0; j < VEC; j++) {
      const float share = by_max ? (s_arg[vi * VEC + j] == t ? to_f<TS>(g0.v[j]) : 0.0f) : to_f<TS>(g0.v[j]) / (float)Tn;
      o.v[j] = from_f<T>(to_f<TS>(g.v[j]) + share);
    }
    *reinterpret_cast<P*>(du + (size_t)t * d + vi * VEC) = o;
  }
}

// the sums over all samples of workgroup k behind the row workgroups: the rows with one key (modal label / embedding row), in row order
template <typename T, typename TS>
__device__ __forceinline__ void fx_sums(const FxArgs& a, const TS* __restrict__ src, int k, int n_groups, float* s_mem, int* s_cnt) {
  const int d = a.d;
  int* s_rows = reinterpret_cast<int*>(s_mem);
  float* s_red = s_mem + FX_MAX_ROWS;
  const int n_modal = a.n >= 2 ? a.n_labels * n_groups : 0;
  if (k < n_modal) {
    const int l = k / n_groups, g = k - l * n_groups;
    if (threadIdx.x == 0) {
      int c = 0;
      for (int s = 0; s < a.S; s++)
        if (a.labels[s] == l) s_rows[c++] = s;
      *s_cnt = c;
    }
    __syncthreads();
    fx_sum_rows<T, TS>(a, src, s_rows, *s_cnt, g, a.d_modal + (size_t)l * d, s_red);
    return;
  }
  if (a.emb_rows <= 0) return;
  const int ke = k - n_modal;
  if (ke < a.S * n_groups) {
    // (memory row s0, column group g): if s0 is the FIRST row that reads its embedding row e, this workgroup sums e's group g
    const int s0 = ke / n_groups, g = ke - s0 * n_groups;
    const int e = a.tidx[s0];
    if ((unsigned)e >= (unsigned)a.emb_rows) return;
    int earlier = 0;
    for (int s = threadIdx.x; s < s0; s += FX_THREADS) earlier |= (a.tidx[s] == e);
    if (__syncthreads_or(earlier)) return;
    if (threadIdx.x == 0) {
      int c = 0;
      for (int s = s0; s < a.S; s++)
        if (a.tidx[s] == e) s_rows[c++] = s;
      *s_cnt = c;
    }
    __syncthreads();
    fx_sum_rows<T, TS>(a, src, s_rows, *s_cnt, g, a.d_emb + (size_t)e * d, s_red);
    return;
  }
  // FX_ZERO_WGS workgroups zero the rows nobody reads: s_rows[e'] = 1 marks the read ones of this workgroup's slice
  const int z = ke - a.S * n_groups;
  const int per = (a.emb_rows + FX_ZERO_WGS - 1) / FX_ZERO_WGS;
  const int e0 = z * per, e1 = min(e0 + per, a.emb_rows);
  for (int e0c = e0; e0c < e1; e0c += FX_MAX_ROWS) {       // (slices of at most FX_MAX_ROWS rows: the flags live in s_rows)
    const int ne = min(e1 - e0c, FX_MAX_ROWS);
    for (int q = threadIdx.x; q < ne; q += FX_THREADS) s_rows[q] = 0;
    __syncthreads();
    for (int s = threadIdx.x; s < a.S; s += FX_THREADS) {
      const int e = a.tidx[s] - e0c;
      if ((unsigned)e < (unsigned)ne) s_rows[e] = 1;       // (every writer stores the same value)
    }
    __syncthreads();
    const int nv = d / 4;
    for (int q = threadIdx.x; q < ne * nv; q += FX_THREADS) {
      const int r = q / nv, c4 = q - r * nv;
      if (!s_rows[r]) *reinterpret_cast<float4*>(a.d_emb + (size_t)(e0c + r) * d + c4 * 4) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    __syncthreads();
  }
}

// nb_rows: the row workgroups in front of this launch's grid (B * n, or 0 in the reductions-only launch behind a norm backward)
template <typename T>
__global__ __launch_bounds__(FX_THREADS) void enc_frontend_ex_bwd_kernel(FxArgs a, int n_groups, int nb_rows) {
  constexpr int VEC = FxCfg<T>::VEC, MAXIT = FxCfg<T>::MAXIT;
  using P = FxPack<T, VEC>;
  __shared__ float s_mem[FX_WAVES * 2 * FX_MAX_D];       // norm: [wave][dgamma | dbeta][column]; reductions: row list + lane partials
  __shared__ int s_arg[FX_MAX_D];
  __shared__ int s_cnt;
  const int d = a.d, nvec = d / VEC;
  if ((int)blockIdx.x < nb_rows) {
    const int b = blockIdx.x / a.n, i = blockIdx.x - b * a.n;
    const int Tn = a.T[i];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t base = (size_t)b * a.S + a.off[i];
    const T* __restrict__ u = static_cast<const T*>(a.u[i]) + (size_t)b * Tn * d;
    const bool by_max = a.agg == VCT_AGG_MAX;
    if (a.norm) {
      const T* __restrict__ dx = static_cast<const T*>(a.dx);
      float* __restrict__ dpre = a.dpre;
      const Dropout dr = make_dropout(a.seed, a.site, a.p_drop);
      float pg[MAXIT][VEC], pb[MAXIT][VEC];
#pragma unroll
      for (int it = 0; it < MAXIT; it++)
#pragma unroll
        for (int j = 0; j < VEC; j++) { pg[it][j] = 0.0f; pb[it][j] = 0.0f; }
      for (int r = wave; r <= Tn; r += FX_WAVES) {
        float v[MAXIT][VEC], gg[MAXIT][VEC];
        int am[MAXIT][VEC];
        fx_pre_row<T>(a, u, Tn, a.off[i] + r, r, lane, v, am);
        const size_t row = base + r;
        const float mean = a.mean[row], rstd = a.rstd[row];
        float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
        for (int it = 0; it < MAXIT; it++) {
          const int vi = it * WAVE + lane;
#pragma unroll
          for (int j = 0; j < VEC; j++) gg[it][j] = 0.0f;
          if (vi < nvec) {
            if (r == 0 && by_max) {
#pragma unroll
              for (int j = 0; j < VEC; j++) s_arg[vi * VEC + j] = am[it][j];
            }
            const P g = *reinterpret_cast<const P*>(dx + row * d + vi * VEC);
            float dm[VEC];
            drop_mults<VEC>(dr, (uint32_t)row * (uint32_t)d + (uint32_t)(vi * VEC), dm);
#pragma unroll
            for (int j = 0; j < VEC; j++) {
              const float gy = to_f<T>(g.v[j]) * dm[j];
              const float xh = (v[it][j] - mean) * rstd;
              const float w = gy * a.gamma[vi * VEC + j];
              v[it][j] = xh; gg[it][j] = w;
              s1 += w; s2 += w * xh;
              pg[it][j] += gy * xh; pb[it][j] += gy;
            }
          }
        }
        const float c1 = wave_sum(s1) / (float)d, c2 = wave_sum(s2) / (float)d;
#pragma unroll
        for (int it = 0; it < MAXIT; it++) {
          const int vi = it * WAVE + lane;
          if (vi < nvec) {
            FxPack<float, VEC> o;
#pragma unroll
            for (int j = 0; j < VEC; j++) o.v[j] = rstd * (gg[it][j] - c1 - v[it][j] * c2);
            *reinterpret_cast<FxPack<float, VEC>*>(dpre + row * d + vi * VEC) = o;
          }
        }
      }
#pragma unroll
      for (int it = 0; it < MAXIT; it++) {
        const int vi = it * WAVE + lane;
        if (vi < nvec) {
#pragma unroll
          for (int j = 0; j < VEC; j++) {
            s_mem[(wave * 2 + 0) * FX_MAX_D + vi * VEC + j] = pg[it][j];
            s_mem[(wave * 2 + 1) * FX_MAX_D + vi * VEC + j] = pb[it][j];
          }
        }
      }
    } else if (by_max && wave == 0) {
      float v[MAXIT][VEC];
      int am[MAXIT][VEC];
      fx_pre_row<T, false>(a, u, Tn, a.off[i], 0, lane, v, am);
#pragma unroll
      for (int it = 0; it < MAXIT; it++) {
        const int vi = it * WAVE + lane;
        if (vi < nvec) {
#pragma unroll
          for (int j = 0; j < VEC; j++) s_arg[vi * VEC + j] = am[it][j];
        }
      }
    }
    __threadfence_block();
    __syncthreads();         // this workgroup's dpre rows, s_arg and the wave partials are complete
    if (a.norm) {
      for (int c = threadIdx.x; c < 2 * d; c += FX_THREADS) {
        const int which = c / d, col = c - which * d;
        float sum = 0.0f;
#pragma unroll
        for (int w = 0; w < FX_WAVES; w++) sum += s_mem[(w * 2 + which) * FX_MAX_D + col];
        a.param_ws[((size_t)blockIdx.x * 2 + which) * d + col] = sum;
      }
    }
    T* __restrict__ du = static_cast<T*>(a.du[i]) + (size_t)b * Tn * d;
    if (a.norm) fx_du_rows<T, float>(a, a.dpre, du, base, Tn, by_max, s_arg);
    else fx_du_rows<T, T>(a, static_cast<const T*>(a.dx), du, base, Tn, by_max, s_arg);
    return;
  }
  const int k = blockIdx.x - nb_rows;
  if (a.norm) fx_sums<T, float>(a, a.dpre, k, n_groups, s_mem, &s_cnt);
  else fx_sums<T, T>(a, static_cast<const T*>(a.dx), k, n_groups, s_mem, &s_cnt);
}

}  // namespace vct
using namespace vct;

static bool fx_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }

// shape / pointer checks shared by both directions; fills the kernel arguments
static int fx_prepare(const vct_enc_frontend_ex_desc* p, bool fwd, FxArgs& a) {
  if (p == nullptr) return VCT_E_ARG;
  if (p->dtype != VCT_F32 && p->dtype != VCT_BF16) return VCT_E_ARG;
  if (p->agg != VCT_AGG_MEAN && p->agg != VCT_AGG_MAX) return VCT_E_ARG;
  if (p->temporal != VCT_TEMPORAL_FIXED && p->temporal != VCT_TEMPORAL_LEARNED) return VCT_E_ARG;
  if (p->n < 1 || p->n > VCT_MM_MAX_MODAL || p->B <= 0 || p->d <= 0 || p->d > FX_MAX_D) return VCT_E_SHAPE;
  if (p->n >= 2 && p->n_labels != p->n && p->n_labels != 2 * p->n) return VCT_E_SHAPE;
  if (p->d % (p->dtype == VCT_BF16 ? 8 : 4)) return VCT_E_ALIGN;
  const bool learned = p->temporal == VCT_TEMPORAL_LEARNED, norm = p->norm != 0, by_max = p->agg == VCT_AGG_MAX;
  if (learned && p->emb_rows <= 0) return VCT_E_SHAPE;
  if (!(p->p_drop >= 0.0f && p->p_drop < 1.0f)) return VCT_E_ARG;
  const bool need_pre = fwd || norm;         // the backward of the norm recomputes pre
  if (p->n >= 2 && p->labels == nullptr) return VCT_E_ARG;
  if (p->n >= 2 && need_pre && p->modal_w == nullptr) return VCT_E_ARG;
  if (learned && (p->tidx == nullptr || (need_pre && p->emb_w == nullptr))) return VCT_E_ARG;
  if (!learned && need_pre && p->temp == nullptr) return VCT_E_ARG;
  if (norm && (!p->gamma || !p->mean || !p->rstd || (fwd && !p->beta))) return VCT_E_ARG;
  if (need_pre && (!fx_aligned(p->temp) || !fx_aligned(p->emb_w) || !fx_aligned(p->modal_w))) return VCT_E_ALIGN;
  a.n = p->n; a.B = p->B; a.d = p->d; a.n_labels = p->n >= 2 ? p->n_labels : 0;
  a.agg = p->agg; a.learned = learned; a.norm = norm; a.emb_rows = learned ? p->emb_rows : 0;
  a.site = p->site; a.p_drop = p->p_drop;
  for (int i = 0; i < VCT_MM_MAX_MODAL; i++) {
    a.T[i] = 0; a.off[i] = 0; a.u[i] = nullptr; a.mask[i] = nullptr; a.du[i] = nullptr;
  }
  int S = 0;
  for (int i = 0; i < p->n; i++) {
    if (p->T[i] <= 0) return VCT_E_SHAPE;
    a.T[i] = p->T[i];
    a.off[i] = S;
    S += p->T[i] + 1;
    if (S > FX_MAX_ROWS) return VCT_E_SHAPE;
    if (need_pre || by_max) {
      if (p->u[i] == nullptr) return VCT_E_ARG;
      if (!fx_aligned(p->u[i])) return VCT_E_ALIGN;
      a.u[i] = p->u[i];
    }
    if (fwd) {
      a.mask[i] = p->mask[i];
    } else {
      if (p->du[i] == nullptr) return VCT_E_ARG;
      if (!fx_aligned(p->du[i])) return VCT_E_ALIGN;
      a.du[i] = p->du[i];
    }
  }
  a.S = S;
  a.temp = p->temp; a.emb_w = p->emb_w; a.tidx = p->tidx; a.modal_w = p->modal_w; a.labels = p->labels;
  a.gamma = p->gamma; a.beta = p->beta; a.seed = p->seed;
  a.x0 = p->x0; a.key_pad = p->key_pad; a.mean = p->mean; a.rstd = p->rstd;
  a.dx = p->dx; a.d_modal = p->d_modal; a.d_emb = p->d_emb; a.dpre = p->dpre; a.param_ws = p->param_ws;
  if (fwd) {
    if (!p->x0) return VCT_E_ARG;
    if (!fx_aligned(p->x0)) return VCT_E_ALIGN;
  } else {
    if (!p->dx || (p->n >= 2 && !p->d_modal) || (learned && !p->d_emb)) return VCT_E_ARG;
    if (norm && (!p->dpre || !p->param_ws)) return VCT_E_ARG;
    if (!fx_aligned(p->dx) || !fx_aligned(p->d_emb) || !fx_aligned(p->dpre)) return VCT_E_ALIGN;
  }
  return VCT_OK;
}

extern "C" int vct_enc_frontend_ex_fwd(const vct_enc_frontend_ex_desc* p, void* stream) {
  FxArgs a;
  const int rc = fx_prepare(p, true, a);
  if (rc != VCT_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (p->dtype == VCT_BF16)
    vct::launch((enc_frontend_ex_fwd_kernel<bf16_t>), dim3(a.B, a.n), dim3(FX_THREADS), 0, st, a);
  else
    vct::launch((enc_frontend_ex_fwd_kernel<float>), dim3(a.B, a.n), dim3(FX_THREADS), 0, st, a);
  VCT_CHECK_LAUNCH();
  return VCT_OK;
}

extern "C" int vct_enc_frontend_ex_bwd(const vct_enc_frontend_ex_desc* p, void* stream) {
  FxArgs a;
  const int rc = fx_prepare(p, false, a);
  if (rc != VCT_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int vec = p->dtype == VCT_BF16 ? 8 : 4;
  const int n_groups = (a.d / vec + FX_CV - 1) / FX_CV;
  const int n_sums = (a.n >= 2 ? a.n_labels * n_groups : 0) + (a.emb_rows > 0 ? a.S * n_groups + FX_ZERO_WGS : 0);
  const int nb_rows = a.B * a.n;
  // with the norm the sums read the dpre of every sample, which the row workgroups of this launch produce: they go behind it
  const int first = nb_rows + (a.norm ? 0 : n_sums);
  if (p->dtype == VCT_BF16)
    vct::launch((enc_frontend_ex_bwd_kernel<bf16_t>), dim3(first), dim3(FX_THREADS), 0, st, a, n_groups, nb_rows);
  else
    vct::launch((enc_frontend_ex_bwd_kernel<float>), dim3(first), dim3(FX_THREADS), 0, st, a, n_groups, nb_rows);
  VCT_CHECK_LAUNCH();
  if (a.norm && n_sums > 0) {
    if (p->dtype == VCT_BF16)
      vct::launch((enc_frontend_ex_bwd_kernel<bf16_t>), dim3(n_sums), dim3(FX_THREADS), 0, st, a, n_groups, 0);
    else
      vct::launch((enc_frontend_ex_bwd_kernel<float>), dim3(n_sums), dim3(FX_THREADS), 0, st, a, n_groups, 0);
    VCT_CHECK_LAUNCH();
  }
  return VCT_OK;
}
