// Ensemble decoding on gfx950: the logits of up to eight models -> one fp32 row of combined log-probabilities per decode row,
// which the controls and selection kernels then treat as the step's logits (a row of log-probabilities is a valid logits row).
//
// replaces: nothing in the reference (it decodes with one checkpoint, MMT4Caption.py:146-184); the semantics are the project's
// (include/vct_hip.h, vct_ensemble_combine; decode.Ensemble).  The weights are read from device memory, so the captured
// per-position graphs serve every weighting.
//
// ONE WORKGROUP PER ROW, 512 threads.  A row of V = 30522 logits per member does not fit a workgroup's registers once there is
// more than one member, so nothing is held: every sweep reads the members' rows again (61 KB fp32 per member at that V -- the
// first read comes from HBM or from the generator's write-back, the later ones from L2).
//   sweep 1, 2   per member with w_m > 0: M_m = max z, then S_m = sum exp(z - M_m); block reductions in a fixed order.  Two
//                sweeps rather than one running (max, sum) pair: the sum then has exactly V terms exp(z - M_m) <= 1 and no
//                rescaling factors, which is what the tests' error bound is derived for.
//   sweep 3      per 8 columns: lp_m = (z - M_m) - log S_m of every active member in registers (member loop unrolled: the
//                indices are compile-time), then the weighted sum (LOGP) or A + log sum w exp(lp - A) (PROB).
// Members of mixed dtype: a thread's unit of work is 8 columns = one 16-byte load of a bf16 member, two of an fp32 member, two
// 16-byte stores of out.  A tensor whose base or row stride breaks 16-byte row alignment is read / written by elements, as is
// the V % 8 tail.  Columns >= V are never touched.  No atomics, no workspace.
#include "vct_common.h"

namespace vct {

constexpr int ENS_NT = 512;
constexpr int ENS_NW = ENS_NT / 64;
constexpr int ENS_COLS = 8;                 // columns per thread and trip

struct EnsArgs {
  const void* x[VCT_ENSEMBLE_MAX];
  int64_t ld[VCT_ENSEMBLE_MAX];
  int32_t dtype[VCT_ENSEMBLE_MAX];
  int32_t vec[VCT_ENSEMBLE_MAX];            // rows of this member are 16-byte aligned
  const float* w;
  float* out;
  int64_t ld_out;
  int32_t n, V, out_vec;
};

// columns c .. c + 7 of a row (all inside [0, V)) as fp32
template <typename T> __device__ __forceinline__ void ens_load8(const T* __restrict__ r, int c, bool vec, float (&z)[ENS_COLS]);
template <> __device__ __forceinline__ void ens_load8<float>(const float* __restrict__ r, int c, bool vec, float (&z)[ENS_COLS]) {
  if (vec) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(r + c), b = *reinterpret_cast<const f32x4*>(r + c + 4);
#pragma unroll
    for (int j = 0; j < 4; j++) { z[j] = a[j]; z[4 + j] = b[j]; }
  } else {
#pragma unroll
    for (int j = 0; j < ENS_COLS; j++) z[j] = r[c + j];
  }
}
template <> __device__ __forceinline__ void ens_load8<bf16_t>(const bf16_t* __restrict__ r, int c, bool vec, float (&z)[ENS_COLS]) {
  if (vec) {
    const s16x8 a = *reinterpret_cast<const s16x8*>(r + c);
#pragma unroll
    for (int j = 0; j < ENS_COLS; j++) z[j] = bf2f((bf16_t)a[j]);
  } else {
#pragma unroll
    for (int j = 0; j < ENS_COLS; j++) z[j] = bf2f(r[c + j]);
  }
}

// this thread's share of max z over the row (fmaxf drops a NaN: the sum below brings it back)
template <typename T> __device__ __forceinline__ float ens_row_max(const T* __restrict__ r, int V, bool vec) {
  float mx = -INFINITY;
  const int Vf = V & ~(ENS_COLS - 1);
  for (int c = threadIdx.x * ENS_COLS; c < Vf; c += ENS_NT * ENS_COLS) {
    float z[ENS_COLS];
    ens_load8<T>(r, c, vec, z);
#pragma unroll
    for (int j = 0; j < ENS_COLS; j++) mx = fmaxf(mx, z[j]);
  }
  if ((int)threadIdx.x < V - Vf) mx = fmaxf(mx, to_f<T>(r[Vf + threadIdx.x]));
  return mx;
}

// this thread's share of sum exp(z - mx)
template <typename T> __device__ __forceinline__ float ens_row_expsum(const T* __restrict__ r, int V, bool vec, float mx) {
  float s = 0.0f;
  const int Vf = V & ~(ENS_COLS - 1);
  for (int c = threadIdx.x * ENS_COLS; c < Vf; c += ENS_NT * ENS_COLS) {
    float z[ENS_COLS];
    ens_load8<T>(r, c, vec, z);
#pragma unroll
    for (int j = 0; j < ENS_COLS; j++) s += __expf(z[j] - mx);
  }
  if ((int)threadIdx.x < V - Vf) s += __expf(to_f<T>(r[Vf + threadIdx.x]) - mx);
  return s;
}

// out of N columns from the active members' lp (member index compile-time: lp stays in registers)
template <int MODE, int N>
__device__ __forceinline__ void ens_mix(const float (&lp)[VCT_ENSEMBLE_MAX][N], const float* __restrict__ s_w, int n, unsigned active,
                                        float (&o)[N]) {
#pragma unroll
  for (int j = 0; j < N; j++) {
    if (MODE == VCT_ENS_LOGP) {
      float acc = 0.0f;
#pragma unroll
      for (int m = 0; m < VCT_ENSEMBLE_MAX; m++)
        if (m < n && ((active >> m) & 1u)) acc = fmaf(s_w[m], lp[m][j], acc);
      o[j] = acc;
    } else {
      float A = -INFINITY;
#pragma unroll
      for (int m = 0; m < VCT_ENSEMBLE_MAX; m++)
        if (m < n && ((active >> m) & 1u)) A = fmaxf(A, lp[m][j]);
      const float ref = A == -INFINITY ? 0.0f : A;          // every lp -inf: the sum is 0 and its log -inf (no inf - inf)
      float sum = 0.0f;
#pragma unroll
      for (int m = 0; m < VCT_ENSEMBLE_MAX; m++)
        if (m < n && ((active >> m) & 1u)) sum = fmaf(s_w[m], __expf(lp[m][j] - ref), sum);      // a NaN lp: fmaxf dropped it, this does not
      o[j] = ref + __logf(sum);
    }
  }
}

template <int MODE>
__global__ __launch_bounds__(ENS_NT) void ensemble_combine_kernel(const EnsArgs a) {
  __shared__ float red[ENS_NW];
  __shared__ float s_M[VCT_ENSEMBLE_MAX], s_L[VCT_ENSEMBLE_MAX], s_w[VCT_ENSEMBLE_MAX];
  const int tid = threadIdx.x, V = a.V, n = a.n;
  const size_t row = blockIdx.x;
  unsigned active = 0;
  // ---- statistics of every active member's row ------------------------------------------------------------------------------
  for (int m = 0; m < n; m++) {
    const float wm = a.w[m];
    if (!(wm > 0.0f)) continue;                               // (uniform over the workgroup)
    active |= 1u << m;
    const bool vec = a.vec[m] != 0;
    float mx, s;
    if (a.dtype[m] == VCT_BF16) {
      const bf16_t* r = (const bf16_t*)a.x[m] + row * (size_t)a.ld[m];
      mx = block_max<ENS_NW>(ens_row_max<bf16_t>(r, V, vec), red);
      s = block_sum<ENS_NW>(ens_row_expsum<bf16_t>(r, V, vec, mx), red);
    } else {
      const float* r = (const float*)a.x[m] + row * (size_t)a.ld[m];
      mx = block_max<ENS_NW>(ens_row_max<float>(r, V, vec), red);
      s = block_sum<ENS_NW>(ens_row_expsum<float>(r, V, vec, mx), red);
    }
    if (tid == 0) { s_M[m] = mx; s_L[m] = logf(s); s_w[m] = wm; }
  }
  __syncthreads();
  // ---- the combination --------------------------------------------------------------------------------------------------------
  float* __restrict__ orow = a.out + row * (size_t)a.ld_out;
  const int Vf = V & ~(ENS_COLS - 1);
  for (int c = tid * ENS_COLS; c < Vf; c += ENS_NT * ENS_COLS) {
    float lp[VCT_ENSEMBLE_MAX][ENS_COLS];
#pragma unroll
    for (int m = 0; m < VCT_ENSEMBLE_MAX; m++) {
      if (m < n && ((active >> m) & 1u)) {
        float z[ENS_COLS];
        if (a.dtype[m] == VCT_BF16) ens_load8<bf16_t>((const bf16_t*)a.x[m] + row * (size_t)a.ld[m], c, a.vec[m] != 0, z);
        else ens_load8<float>((const float*)a.x[m] + row * (size_t)a.ld[m], c, a.vec[m] != 0, z);
        const float M = s_M[m], L = s_L[m];
#pragma unroll
        for (int j = 0; j < ENS_COLS; j++) lp[m][j] = (z[j] - M) - L;
      }
    }
    float o[ENS_COLS];
    ens_mix<MODE, ENS_COLS>(lp, s_w, n, active, o);
    if (a.out_vec) {
      f32x4 lo, hi;
#pragma unroll
      for (int j = 0; j < 4; j++) { lo[j] = o[j]; hi[j] = o[4 + j]; }
      *reinterpret_cast<f32x4*>(orow + c) = lo;
      *reinterpret_cast<f32x4*>(orow + c + 4) = hi;
    } else {
#pragma unroll
      for (int j = 0; j < ENS_COLS; j++) orow[c + j] = o[j];
    }
  }
  if (tid < V - Vf) {                                         // the V % 8 tail: one column per thread
    const int c = Vf + tid;
    float lp[VCT_ENSEMBLE_MAX][1];
#pragma unroll
    for (int m = 0; m < VCT_ENSEMBLE_MAX; m++) {
      if (m < n && ((active >> m) & 1u)) {
        const float z = a.dtype[m] == VCT_BF16 ? bf2f(((const bf16_t*)a.x[m] + row * (size_t)a.ld[m])[c])
                                               : ((const float*)a.x[m] + row * (size_t)a.ld[m])[c];
        lp[m][0] = (z - s_M[m]) - s_L[m];
      }
    }
    float o[1];
    ens_mix<MODE, 1>(lp, s_w, n, active, o);
    orow[c] = o[0];
  }
}

}  // namespace vct
using namespace vct;

extern "C" int vct_ensemble_combine(const vct_ensemble_desc* d, void* stream) {
  if (!d) return VCT_E_ARG;
  if (d->n < 1 || d->n > VCT_ENSEMBLE_MAX) return VCT_E_SHAPE;     // (before the member arrays are walked)
  if (!d->w || !d->out || (d->mode != VCT_ENS_PROB && d->mode != VCT_ENS_LOGP)) return VCT_E_ARG;
  for (int m = 0; m < d->n; m++)
    if (!d->x[m] || (d->dtype[m] != VCT_F32 && d->dtype[m] != VCT_BF16)) return VCT_E_ARG;
  if (d->rows < 1 || d->V < 1 || d->ld_out < d->V) return VCT_E_SHAPE;
  for (int m = 0; m < d->n; m++)
    if (d->ld[m] < d->V) return VCT_E_SHAPE;
  EnsArgs a = {};
  auto rows_aligned = [&](const void* p, int64_t ld, int64_t esize) {
    return ((uintptr_t)p % 16 == 0 && (d->rows == 1 || (ld * esize) % 16 == 0)) ? 1 : 0;
  };
  for (int m = 0; m < d->n; m++) {
    a.x[m] = d->x[m];
    a.ld[m] = d->ld[m];
    a.dtype[m] = d->dtype[m];
    a.vec[m] = rows_aligned(d->x[m], d->ld[m], d->dtype[m] == VCT_BF16 ? 2 : 4);
  }
  a.w = d->w;
  a.out = d->out;
  a.ld_out = d->ld_out;
  a.n = d->n;
  a.V = d->V;
  a.out_vec = rows_aligned(d->out, d->ld_out, 4);
  const dim3 grid(d->rows), block(ENS_NT);
  hipStream_t st = (hipStream_t)stream;
  if (d->mode == VCT_ENS_LOGP) vct::launch((ensemble_combine_kernel<VCT_ENS_LOGP>), grid, block, 0, st, a);
  else vct::launch((ensemble_combine_kernel<VCT_ENS_PROB>), grid, block, 0, st, a);
  VCT_CHECK_LAUNCH();
  return VCT_OK;
}
