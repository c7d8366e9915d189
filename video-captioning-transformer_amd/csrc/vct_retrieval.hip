// Text-video retrieval evaluation of the matching head on gfx950 (include/vct_hip.h: vct_retrieval_ranks).
//
// The [Nt, Nv] score matrix f is never stored: ranks are counts, so every 128 x 128 tile of it is computed (fp32 MFMA), compared
// against the ground-truth scores of its rows and columns and thrown away.
//
//   1 ret_prep_kernel     one wave per row: 1 / |t_i|, 1 / |v_j| (fixed order); zeroes the counters and the per-video best keys
//   2 ret_sweep<STATS>    dual-softmax only: per tile and column the max and the sum of exp of s / tau over the tile's rows
//     ret_colstat_kernel  one thread per column folds the row-tile partials in tile order: max and log-sum-exp
//   3 ret_gt_kernel       one wave per 16 texts: f[i, gt[i]] through the SAME MFMA chain as the sweep (a 16 x 16 tile against the
//                         gathered video rows, of which the diagonal is kept); the best own text of every video by an integer
//                         atomicMax on (ordered score bits, ~index)
//   4 ret_sweep<COUNT>    every tile once: the text->video counts of its rows and the video->text counts of its columns (LDS integer
//                         atomics, then one global integer atomic per row / column that has something to add)
//   5 ret_finish_kernel   ONE workgroup: counts -> ranks, recall at 1 / 5 / 10, mean, and the median by a two-level rank histogram in LDS
//
// One definition of f[i, j].  raw[i, j] is one fmaf chain over k in a fixed order (tile_product and gt_product issue the same
// v_mfma_f32_16x16x4_f32 sequence: K chunks of 16 ascending, inside a chunk k = 4 g + q for q = 0..3, g = 0..3), independent of the
// tile position and of Nt / Nv; s = (raw * rt[i]) * rv[j]; ret_score turns s into f with explicit fmaf / single products only.  So
// the `>` and `==` of the rank definitions compare like with like.  No floating-point atomic, no data-dependent order of a
// floating-point sum: two calls on the same inputs agree bitwise.
#include "vct_common.h"
#include <math.h>

namespace vct {

constexpr int RT_THREADS = 256;
constexpr int RT_BM = 128, RT_BN = 128;     // texts x videos per tile; 2 x 2 waves of 64 x 64
constexpr int RT_BK = 32;
constexpr int RT_STR = RT_BK + 4;           // LDS row stride (floats): rows 0..15 of a 16-byte read land on distinct bank quads
constexpr int RT_MAX_D = 1024;
constexpr int RT_MAX_N = 1 << 20;
constexpr int RT_FIN_THREADS = 1024;

enum { RT_PH_PREP = 1, RT_PH_STATS = 2, RT_PH_GT = 4, RT_PH_COUNT = 8, RT_PH_FINISH = 16, RT_PH_ALL = 31 };

struct RetWs {
  float* rt;                   // [Nt] 1 / |t_i|
  float* rv;                   // [Nv] 1 / |v_j|
  float* fgt;                  // [Nt] f[i, gt[i]]
  int* gv;                     // [Nt] gt[i], or -1 when it is outside [0, Nv)
  unsigned long long* best;    // [Nv] (ordered bits of f[i*, j]) << 32 | ~i*; 0: the video has no text
  float* cm;                   // [Nv] dual softmax: max_i s[i, j] / tau
  float* cl;                   // [Nv] dual softmax: log sum_i exp(s[i, j] / tau - cm[j])
  float2* part;                // [row tiles, Nv] dual softmax: the per-tile (max, sum)
};

__host__ __device__ inline size_t ret_up16(size_t b) { return (b + 15) & ~(size_t)15; }

__host__ inline size_t ret_ws_layout(char* base, int Nt, int Nv, int mode, RetWs* w) {
  size_t at = 0;
  auto take = [&](size_t bytes) { char* p = base + at; at += ret_up16(bytes); return p; };
  RetWs l;
  l.rt = (float*)take(4 * (size_t)Nt);
  l.rv = (float*)take(4 * (size_t)Nv);
  l.fgt = (float*)take(4 * (size_t)Nt);
  l.gv = (int*)take(4 * (size_t)Nt);
  l.best = (unsigned long long*)take(8 * (size_t)Nv);
  l.cm = l.cl = nullptr;
  l.part = nullptr;
  if (mode == VCT_RETRIEVAL_DUAL_SOFTMAX) {
    l.cm = (float*)take(4 * (size_t)Nv);
    l.cl = (float*)take(4 * (size_t)Nv);
    l.part = (float2*)take(8 * (size_t)((Nt + RT_BM - 1) / RT_BM) * (size_t)Nv);
  }
  if (w != nullptr) *w = l;
  return at;
}

// f from s.  Dual softmax: s * exp(s / tau - cm[j] - cl[j]); one explicit fma, one subtraction, single products.
template <int MODE> __device__ __forceinline__ float ret_score(float s, float inv_tau, float cm, float cl) {
  if constexpr (MODE == VCT_RETRIEVAL_PLAIN) return s;
  const float z = fmaf(s, inv_tau, -cm);
  return s * expf(z - cl);
}

// an order-preserving map of a float's bits (-0 counts as +0, so that a tie between them goes to the lower index)
__device__ __forceinline__ uint32_t ret_ordered(float f) {
  const uint32_t b = __float_as_uint(f + 0.0f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float ret_unordered(uint32_t o) {
  return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

__global__ __launch_bounds__(RT_THREADS) void ret_prep_kernel(const float* __restrict__ text, long long ldt, const float* __restrict__ vid,
                                                              long long ldv, int Nt, int Nv, int Dt, RetWs w, int* __restrict__ cnt_t,
                                                              int* __restrict__ cnt_v) {
  const long long gid = (long long)blockIdx.x * RT_THREADS + threadIdx.x;
  if (gid < Nt) cnt_t[gid] = 0;
  if (gid < Nv) { cnt_v[gid] = 0; w.best[gid] = 0ull; }
  const long long row = gid >> 6;                             // one wave per row: texts first, then videos
  const int lane = threadIdx.x & 63;
  if (row >= (long long)Nt + Nv) return;                      // (uniform over the wave)
  const bool is_t = row < Nt;
  const float* x = is_t ? text + (size_t)row * ldt : vid + (size_t)(row - Nt) * ldv;
  float a = 0.0f;
  for (int k = 4 * lane; k < Dt; k += 4 * WAVE) {
    const float4 v = *reinterpret_cast<const float4*>(x + k);
    a = fmaf(v.x, v.x, a); a = fmaf(v.y, v.y, a); a = fmaf(v.z, v.z, a); a = fmaf(v.w, v.w, a);
  }
  a = wave_sum(a);
  if (lane == 0) (is_t ? w.rt[row] : w.rv[row - Nt]) = 1.0f / sqrtf(a);
}

constexpr int RT_LOAD_NV = RT_BM * RT_BK / 4 / RT_THREADS;    // 16-byte vectors per thread and operand of one K tile

__device__ __forceinline__ void tile_load(float4 (&ra)[RT_LOAD_NV], float4 (&rb)[RT_LOAD_NV], const float* __restrict__ text, long long ldt,
                                          const float* __restrict__ vid, long long ldv, int i0, int j0, int Nt, int Nv, int Dt, int k0) {
#pragma unroll
  for (int u = 0; u < RT_LOAD_NV; u++) {
    const int v = threadIdx.x + u * RT_THREADS, row = v >> 3, k = k0 + (v & 7) * 4;
    // (Dt is a multiple of 4: a vector is inside the row or outside it)
    ra[u] = rb[u] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (i0 + row < Nt && k < Dt) ra[u] = *reinterpret_cast<const float4*>(text + (size_t)(i0 + row) * ldt + k);
    if (j0 + row < Nv && k < Dt) rb[u] = *reinterpret_cast<const float4*>(vid + (size_t)(j0 + row) * ldv + k);
  }
}

// raw[i0 .. i0 + 127, j0 .. j0 + 127]: acc[ti][tj][r] = row wm * 64 + ti * 16 + (lane >> 4) * 4 + r, column wn * 64 + tj * 16 + (lane & 15)
__device__ __forceinline__ void tile_product(f32x4 (&acc)[4][4], const float* __restrict__ text, long long ldt,
                                             const float* __restrict__ vid, long long ldv, int i0, int j0, int Nt, int Nv, int Dt,
                                             float* la, float* lb) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, i16 = lane & 15, g = lane >> 4;
  constexpr int NV = RT_LOAD_NV;
  float4 ra[NV], rb[NV];
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) acc[i][j] = f32x4{0, 0, 0, 0};
  tile_load(ra, rb, text, ldt, vid, ldv, i0, j0, Nt, Nv, Dt, 0);
  for (int k0 = 0; k0 < Dt; k0 += RT_BK) {
    __syncthreads();                                          // the previous tile's fragment reads are done
#pragma unroll
    for (int u = 0; u < NV; u++) {
      const int v = tid + u * RT_THREADS, row = v >> 3, kc = (v & 7) * 4;
      *reinterpret_cast<float4*>(la + row * RT_STR + kc) = ra[u];
      *reinterpret_cast<float4*>(lb + row * RT_STR + kc) = rb[u];
    }
    __syncthreads();
    if (k0 + RT_BK < Dt) tile_load(ra, rb, text, ldt, vid, ldv, i0, j0, Nt, Nv, Dt, k0 + RT_BK);                  // the next tile's loads fly under the MFMAs
#pragma unroll
    for (int h = 0; h < RT_BK / 16; h++) {
      f32x4 fa[4], fb[4];
#pragma unroll
      for (int t = 0; t < 4; t++) {
        fa[t] = *reinterpret_cast<const f32x4*>(la + (wm * 64 + t * 16 + i16) * RT_STR + h * 16 + 4 * g);
        fb[t] = *reinterpret_cast<const f32x4*>(lb + (wn * 64 + t * 16 + i16) * RT_STR + h * 16 + 4 * g);
      }
#pragma unroll
      for (int q = 0; q < 4; q++)
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
          for (int j = 0; j < 4; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[i][q], fb[j][q], acc[i][j], 0, 0, 0);
    }
  }
}

// The same chain for ONE 16 x 16 tile whose operand rows come straight from global memory: lane (i16, g) owns row i16 of both sides.
__device__ __forceinline__ f32x4 gt_product(const float* __restrict__ trow, const float* __restrict__ vrow, int Dt, int g) {
  f32x4 acc = f32x4{0, 0, 0, 0};
  for (int k0 = 0; k0 < Dt; k0 += 16) {
    const int k = k0 + 4 * g;
    f32x4 a = f32x4{0, 0, 0, 0}, b = a;
    if (k < Dt) {
      a = *reinterpret_cast<const f32x4*>(trow + k);
      b = *reinterpret_cast<const f32x4*>(vrow + k);
    }
#pragma unroll
    for (int q = 0; q < 4; q++) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[q], b[q], acc, 0, 0, 0);
  }
  return acc;
}

template <int MODE>
__global__ __launch_bounds__(RT_THREADS) void ret_gt_kernel(const float* __restrict__ text, long long ldt, const float* __restrict__ vid,
                                                            long long ldv, const int* __restrict__ gt, const float* __restrict__ tau,
                                                            int Nt, int Nv, int Dt, RetWs w) {
  const int lane = threadIdx.x & 63, i16 = lane & 15, g = lane >> 4;
  const long long i = ((long long)blockIdx.x * (RT_THREADS / WAVE) + (threadIdx.x >> 6)) * 16 + i16;
  const bool in = i < Nt;
  const int gi = in ? gt[i] : -1;
  const bool ok = in && gi >= 0 && gi < Nv;                   // a gt outside the videos is never used as an index
  const float* trow = text + (size_t)(in ? i : 0) * ldt;
  const float* vrow = vid + (size_t)(ok ? gi : 0) * ldv;
  const f32x4 acc = gt_product(trow, vrow, Dt, g);            // (every lane of the wave takes part in the MFMAs)
  const int r = i16 - 4 * g;                                  // the diagonal: column i16 == row 4 g + r
  if (r < 0 || r > 3 || !in) return;
  w.gv[i] = ok ? gi : -1;
  float f = 0.0f;
  if (ok) {
    const float s = (acc[r] * w.rt[i]) * w.rv[gi];
    float inv_tau = 0.0f, cm = 0.0f, cl = 0.0f;
    if constexpr (MODE == VCT_RETRIEVAL_DUAL_SOFTMAX) { inv_tau = 1.0f / tau[0]; cm = w.cm[gi]; cl = w.cl[gi]; }
    f = ret_score<MODE>(s, inv_tau, cm, cl);
    atomicMax(&w.best[gi], ((unsigned long long)ret_ordered(f) << 32) | (unsigned long long)(~(uint32_t)i));
  }
  w.fgt[i] = f;
}

constexpr int RT_STATS = 0, RT_COUNT = 1;

template <int MODE, int PASS>
__global__ __launch_bounds__(RT_THREADS) void ret_sweep_kernel(const float* __restrict__ text, long long ldt, const float* __restrict__ vid,
                                                               long long ldv, const float* __restrict__ tau, int Nt, int Nv, int Dt,
                                                               RetWs w, int* __restrict__ cnt_t, int* __restrict__ cnt_v) {
  __shared__ __attribute__((aligned(16))) float la[RT_BM * RT_STR];
  __shared__ __attribute__((aligned(16))) float lb[RT_BN * RT_STR];
  __shared__ float s_rt[RT_BM], s_rv[RT_BN], s_fgt[RT_BM], s_fb[RT_BN], s_cm[RT_BN], s_cl[RT_BN];
  __shared__ int s_g[RT_BM], s_ib[RT_BN], s_ct[RT_BM], s_cv[RT_BN];
  __shared__ float s_red[2][RT_BN];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, i16 = lane & 15, g = lane >> 4;
  const int i0 = blockIdx.y * RT_BM, j0 = blockIdx.x * RT_BN;
  if (tid < RT_BM) {
    const int i = i0 + tid;
    s_rt[tid] = i < Nt ? w.rt[i] : 0.0f;
    if constexpr (PASS == RT_COUNT) {
      s_fgt[tid] = i < Nt ? w.fgt[i] : 0.0f;
      s_g[tid] = i < Nt ? w.gv[i] : -1;
      s_ct[tid] = 0;
    }
  } else {
    const int c = tid - RT_BM, j = j0 + c;
    s_rv[c] = j < Nv ? w.rv[j] : 0.0f;
    if constexpr (PASS == RT_COUNT) {
      const unsigned long long key = j < Nv ? w.best[j] : 0ull;
      s_fb[c] = ret_unordered((uint32_t)(key >> 32));
      s_ib[c] = key != 0ull ? (int)(~(uint32_t)key) : -1;
      s_cv[c] = 0;
      if constexpr (MODE == VCT_RETRIEVAL_DUAL_SOFTMAX) {
        s_cm[c] = j < Nv ? w.cm[j] : 0.0f;
        s_cl[c] = j < Nv ? w.cl[j] : 0.0f;
      }
    }
  }
  f32x4 acc[4][4];
  tile_product(acc, text, ldt, vid, ldv, i0, j0, Nt, Nv, Dt, la, lb);   // (its first barrier publishes the arrays above)
  float inv_tau = 0.0f;
  if constexpr (MODE == VCT_RETRIEVAL_DUAL_SOFTMAX) inv_tau = 1.0f / tau[0];

  if constexpr (PASS == RT_STATS) {
    // per column of the tile: m = max over its rows of s / tau, then the sum of exp(s / tau - m) in a fixed order: the lane's 16 rows
    // in (ti, r) order, a butterfly over the four lane groups, then the two wave rows in order
    float z[4][4][4], m[4];
#pragma unroll
    for (int tj = 0; tj < 4; tj++) m[tj] = -INFINITY;
#pragma unroll
    for (int ti = 0; ti < 4; ti++)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int row = wm * 64 + ti * 16 + g * 4 + r;
        const bool on = i0 + row < Nt;
        const float rt = s_rt[row];
#pragma unroll
        for (int tj = 0; tj < 4; tj++) {
          const float s = (acc[ti][tj][r] * rt) * s_rv[wn * 64 + tj * 16 + i16];
          const float zz = on ? s * inv_tau : -INFINITY;
          z[ti][tj][r] = zz;
          m[tj] = fmaxf(m[tj], zz);
        }
      }
#pragma unroll
    for (int tj = 0; tj < 4; tj++) {
      m[tj] = fmaxf(m[tj], __shfl_xor(m[tj], 16));
      m[tj] = fmaxf(m[tj], __shfl_xor(m[tj], 32));
      if (g == 0) s_red[wm][wn * 64 + tj * 16 + i16] = m[tj];
    }
    __syncthreads();
    float sum[4];
#pragma unroll
    for (int tj = 0; tj < 4; tj++) {
      const int c = wn * 64 + tj * 16 + i16;
      m[tj] = fmaxf(s_red[0][c], s_red[1][c]);
      if (g == 0 && wm == 0) s_cm[c] = m[tj];                 // (this pass keeps the tile's maxima here)
      sum[tj] = 0.0f;
    }
#pragma unroll
    for (int ti = 0; ti < 4; ti++)
#pragma unroll
      for (int r = 0; r < 4; r++)
#pragma unroll
        for (int tj = 0; tj < 4; tj++) sum[tj] += expf(z[ti][tj][r] - m[tj]);      // (a padding row: exp(-inf) = 0)
    __syncthreads();                                          // everyone has read the maxima
#pragma unroll
    for (int tj = 0; tj < 4; tj++) {
      sum[tj] += __shfl_xor(sum[tj], 16);
      sum[tj] += __shfl_xor(sum[tj], 32);
      if (g == 0) s_red[wm][wn * 64 + tj * 16 + i16] = sum[tj];
    }
    __syncthreads();
    if (tid < RT_BN && j0 + tid < Nv) {
      const int c = tid;
      w.part[(size_t)blockIdx.y * Nv + j0 + c] = make_float2(s_cm[c], s_red[0][c] + s_red[1][c]);
    }
  } else {
    int ct[4][4], cv[4];
#pragma unroll
    for (int tj = 0; tj < 4; tj++) cv[tj] = 0;
#pragma unroll
    for (int ti = 0; ti < 4; ti++)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int row = wm * 64 + ti * 16 + g * 4 + r, gi = i0 + row;
        const float rt = s_rt[row], fg = s_fgt[row];
        const int gg = s_g[row];                              // -1: no valid ground truth, or a padding row
        const bool row_in = gi < Nt;
        int c_row = 0;
#pragma unroll
        for (int tj = 0; tj < 4; tj++) {
          const int col = wn * 64 + tj * 16 + i16, gj = j0 + col;
          const float s = (acc[ti][tj][r] * rt) * s_rv[col];
          float cm = 0.0f, cl = 0.0f;
          if constexpr (MODE == VCT_RETRIEVAL_DUAL_SOFTMAX) { cm = s_cm[col]; cl = s_cl[col]; }
          const float f = ret_score<MODE>(s, inv_tau, cm, cl);
          const bool t_hit = gg >= 0 && gj < Nv && gj != gg && (f > fg || (f == fg && gj < gg));
          c_row += t_hit ? 1 : 0;
          const int ib = s_ib[col];                           // -1: the video has no text, or a padding column
          const float fb = s_fb[col];
          const bool v_hit = ib >= 0 && row_in && gi != ib && (f > fb || (f == fb && gi < ib));
          cv[tj] += v_hit ? 1 : 0;
        }
        ct[ti][r] = c_row;
      }
#pragma unroll
    for (int ti = 0; ti < 4; ti++)
#pragma unroll
      for (int r = 0; r < 4; r++)
        if (ct[ti][r]) atomicAdd(&s_ct[wm * 64 + ti * 16 + g * 4 + r], ct[ti][r]);
#pragma unroll
    for (int tj = 0; tj < 4; tj++)
      if (cv[tj]) atomicAdd(&s_cv[wn * 64 + tj * 16 + i16], cv[tj]);
    __syncthreads();
    if (tid < RT_BM) {
      if (s_ct[tid] && i0 + tid < Nt) atomicAdd(&cnt_t[i0 + tid], s_ct[tid]);
    } else {
      const int c = tid - RT_BM;
      if (s_cv[c] && j0 + c < Nv) atomicAdd(&cnt_v[j0 + c], s_cv[c]);
    }
  }
}

__global__ __launch_bounds__(RT_THREADS) void ret_colstat_kernel(int Nv, int nbi, RetWs w) {
  const int j = blockIdx.x * RT_THREADS + threadIdx.x;
  if (j >= Nv) return;
  float m = -INFINITY;
  for (int b = 0; b < nbi; b++) m = fmaxf(m, w.part[(size_t)b * Nv + j].x);
  float s = 0.0f;
  for (int b = 0; b < nbi; b++) {                             // tile order
    const float2 p = w.part[(size_t)b * Nv + j];
    s = fmaf(p.y, expf(p.x - m), s);
  }
  w.cm[j] = m;
  w.cl[j] = logf(s);
}

// k-th smallest (0-based) of the non-zero ranks in r[0 .. n): a 1024-bin histogram of (rank - 1) >> 10, then one of the low 10 bits
// inside the bin that holds it.  Integer LDS atomics only.
__device__ int ret_select(const int* __restrict__ r, int n, long long k, int* hist, int* pick) {
  const int t = threadIdx.x;
  int coarse = 0;
  for (int level = 0; level < 2; level++) {
    __syncthreads();
    hist[t] = 0;
    __syncthreads();
    for (int i = t; i < n; i += RT_FIN_THREADS) {
      const int v = r[i] - 1;
      if (v < 0) continue;
      if (level == 0) atomicAdd(&hist[min(v >> 10, RT_FIN_THREADS - 1)], 1);    // (a rank is <= 2^20; a phase run alone may see more)
      else if ((v >> 10) == coarse) atomicAdd(&hist[v & 1023], 1);
    }
    __syncthreads();
    if (t == 0) {
      long long left = k;
      int b = 0;
      while (b < 1023 && left >= hist[b]) { left -= hist[b]; b++; }
      pick[0] = b;
      pick[1] = (int)left;
    }
    __syncthreads();
    if (level == 0) { coarse = pick[0]; k = pick[1]; }
  }
  return (coarse << 10) + pick[0] + 1;
}

__global__ __launch_bounds__(RT_FIN_THREADS) void ret_finish_kernel(int Nt, int Nv, RetWs w, int* __restrict__ rank_t, int* __restrict__ rank_v,
                                                                    double* __restrict__ out) {
  __shared__ int hist[RT_FIN_THREADS];
  __shared__ int pick[2];
  __shared__ unsigned long long tot[5];                       // n, sum of ranks, ranks <= 1, <= 5, <= 10
  const int t = threadIdx.x;
  for (int dir = 0; dir < 2; dir++) {
    int* r = dir == 0 ? rank_t : rank_v;
    const int n = dir == 0 ? Nt : Nv;
    __syncthreads();
    if (t < 5) tot[t] = 0ull;
    __syncthreads();
    unsigned long long cnt = 0, sum = 0, r1 = 0, r5 = 0, r10 = 0;
    for (int i = t; i < n; i += RT_FIN_THREADS) {
      const bool valid = dir == 0 ? w.gv[i] >= 0 : w.best[i] != 0ull;
      const int rk = valid ? r[i] + 1 : 0;
      r[i] = rk;
      if (valid) { cnt++; sum += (unsigned long long)rk; r1 += rk <= 1; r5 += rk <= 5; r10 += rk <= 10; }
    }
    if (cnt) {
      atomicAdd(&tot[0], cnt); atomicAdd(&tot[1], sum); atomicAdd(&tot[2], r1); atomicAdd(&tot[3], r5); atomicAdd(&tot[4], r10);
    }
    __syncthreads();                                          // (also: this workgroup's rank stores are visible to its own later reads)
    const long long q = (long long)tot[0];
    double med = 0.0;
    if (q > 0) {                                              // (uniform)
      const int lo = ret_select(r, n, (q - 1) / 2, hist, pick);
      const int hi = ret_select(r, n, q / 2, hist, pick);
      med = 0.5 * ((double)lo + (double)hi);
    }
    if (t == 0) {
      double* o = out + 6 * dir;
      const double dq = (double)q;
      o[0] = q > 0 ? (double)tot[2] / dq : 0.0;
      o[1] = q > 0 ? (double)tot[3] / dq : 0.0;
      o[2] = q > 0 ? (double)tot[4] / dq : 0.0;
      o[3] = med;
      o[4] = q > 0 ? (double)tot[1] / dq : 0.0;
      o[5] = dq;
    }
  }
}

}  // namespace vct
using namespace vct;

static bool rt_shape_ok(int Nt, int Nv, int Dt) {
  return Nt >= 1 && Nt <= RT_MAX_N && Nv >= 1 && Nv <= RT_MAX_N && Dt >= 4 && Dt <= RT_MAX_D && Dt % 4 == 0;
}

extern "C" int64_t vct_retrieval_workspace_bytes(int Nt, int Nv, int Dt, int mode) {
  if (!rt_shape_ok(Nt, Nv, Dt) || (mode != VCT_RETRIEVAL_PLAIN && mode != VCT_RETRIEVAL_DUAL_SOFTMAX)) return 0;
  return (int64_t)ret_ws_layout(nullptr, Nt, Nv, mode, nullptr);
}

template <int MODE>
static int ret_run(const vct_retrieval_desc* p, const RetWs& w, int phases, hipStream_t st) {
  const int Nt = p->Nt, Nv = p->Nv, Dt = p->Dt;
  const long long ldt = p->ld_text, ldv = p->ld_vid;
  const dim3 tiles((unsigned)((Nv + RT_BN - 1) / RT_BN), (unsigned)((Nt + RT_BM - 1) / RT_BM));
  if (phases & RT_PH_PREP) {
    const long long rows = (long long)Nt + Nv;
    vct::launch(ret_prep_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(RT_THREADS), 0, st, p->text, ldt, p->vid, ldv, Nt, Nv, Dt, w,
                p->ranks_t2v, p->ranks_v2t);
    VCT_CHECK_LAUNCH();
  }
  if (MODE == VCT_RETRIEVAL_DUAL_SOFTMAX && (phases & RT_PH_STATS)) {
    vct::launch((ret_sweep_kernel<MODE, RT_STATS>), tiles, dim3(RT_THREADS), 0, st, p->text, ldt, p->vid, ldv, p->tau, Nt, Nv, Dt, w,
                p->ranks_t2v, p->ranks_v2t);
    VCT_CHECK_LAUNCH();
    vct::launch(ret_colstat_kernel, dim3((unsigned)((Nv + RT_THREADS - 1) / RT_THREADS)), dim3(RT_THREADS), 0, st, Nv, (int)tiles.y, w);
    VCT_CHECK_LAUNCH();
  }
  if (phases & RT_PH_GT) {
    vct::launch((ret_gt_kernel<MODE>), dim3((unsigned)((Nt + 63) / 64)), dim3(RT_THREADS), 0, st, p->text, ldt, p->vid, ldv, p->gt, p->tau,
                Nt, Nv, Dt, w);
    VCT_CHECK_LAUNCH();
  }
  if (phases & RT_PH_COUNT) {
    vct::launch((ret_sweep_kernel<MODE, RT_COUNT>), tiles, dim3(RT_THREADS), 0, st, p->text, ldt, p->vid, ldv, p->tau, Nt, Nv, Dt, w,
                p->ranks_t2v, p->ranks_v2t);
    VCT_CHECK_LAUNCH();
  }
  if (phases & RT_PH_FINISH) {
    vct::launch(ret_finish_kernel, dim3(1), dim3(RT_FIN_THREADS), 0, st, Nt, Nv, w, p->ranks_t2v, p->ranks_v2t, p->out);
    VCT_CHECK_LAUNCH();
  }
  return VCT_OK;
}

extern "C" int vct_retrieval_ranks(const vct_retrieval_desc* p, void* stream) {
  if (p == nullptr) return VCT_E_ARG;
  if (p->mode != VCT_RETRIEVAL_PLAIN && p->mode != VCT_RETRIEVAL_DUAL_SOFTMAX) return VCT_E_ARG;
  if ((p->mode == VCT_RETRIEVAL_DUAL_SOFTMAX) != (p->tau != nullptr)) return VCT_E_ARG;
  if (!p->text || !p->vid || !p->gt || !p->ranks_t2v || !p->ranks_v2t || !p->out || !p->workspace) return VCT_E_ARG;
  if (p->phases < 0 || p->phases > RT_PH_ALL) return VCT_E_ARG;
  if (!rt_shape_ok(p->Nt, p->Nv, p->Dt)) return VCT_E_SHAPE;
  if (p->ld_text < p->Dt || p->ld_vid < p->Dt) return VCT_E_SHAPE;
  if (p->ld_text % 4 || p->ld_vid % 4) return VCT_E_ALIGN;
  if (((uintptr_t)p->text & 15) || ((uintptr_t)p->vid & 15) || ((uintptr_t)p->workspace & 15) || ((uintptr_t)p->out & 7) ||
      ((uintptr_t)p->gt & 3) || ((uintptr_t)p->ranks_t2v & 3) || ((uintptr_t)p->ranks_v2t & 3))
    return VCT_E_ALIGN;
  if (p->workspace_bytes < vct_retrieval_workspace_bytes(p->Nt, p->Nv, p->Dt, p->mode)) return VCT_E_WORKSPACE;
  RetWs w;
  ret_ws_layout((char*)p->workspace, p->Nt, p->Nv, p->mode, &w);
  const int phases = p->phases == 0 ? RT_PH_ALL : p->phases;
  hipStream_t st = (hipStream_t)stream;
  return p->mode == VCT_RETRIEVAL_PLAIN ? ret_run<VCT_RETRIEVAL_PLAIN>(p, w, phases, st) : ret_run<VCT_RETRIEVAL_DUAL_SOFTMAX>(p, w, phases, st);
}
