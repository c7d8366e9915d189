// Multi-modal encoder front end on gfx950: the n >= 2 feature streams' unify outputs -> the stack input and its key padding,
// and the backward of that (include/vct_hip.h, vct_mm_frontend_*).
//
// replaces: GlobalAggregation('avg') + cat + TemporalEncoding + ModalEmbedding + the `temp + modal + feats` add of the
// reference's MultiModalEncoder.forward (model/MMEncoder.py:12-48, 83-104, 244-276) for n >= 2 modalities, and the mask cat
// (:252-266).  Memory row layout: modality i owns rows off_i .. off_i + T_i (off_i = sum_{j<i} (T_j + 1)), its aggregation row
// first.
//
// fwd, one launch, grid (B, n), 256 threads: workgroup (b, i) writes modality i's block of sample b --
//   agg row   x0 = (temp[off_i] + modal[label]) + mean_t u_i[b, t]        (fp32 sum over ALL T_i rows, pads included)
//   row t     x0 = (temp[off_i+1+t] + modal[label]) + u_i[b, t]
// and the key-padding bytes of those rows (agg row 0, frame rows = mask_i).
// bwd, one launch, two kinds of workgroups:
//   [0, B*n)        (b, i): du_i[b, t] = dx[b, off_i+1+t] + dx[b, off_i] / T_i
//   [B*n, ...)      (label l, column group g): d_modal[l, g's columns] = sum over the (b, s) pairs with labels[s] == l of
//                   dx[b, s] -- 64 row lanes each sum a fixed residue class of those pairs in order, then the 64 lane partials
//                   are summed in lane order.  No atomics: bitwise reproducible run to run.
#include "vct_common.h"

namespace vct {

constexpr int MM_THREADS = 256;
constexpr int MM_CV = 4;                          // 16-byte column vectors per d_modal workgroup
constexpr int MM_LANES = MM_THREADS / MM_CV;      // row lanes per d_modal workgroup
constexpr int MM_MAX_ROWS = 1024;                 // S limit (the per-label row list lives in LDS)

template <typename T> struct MV { static constexpr int VEC = 16 / sizeof(T); };
template <typename T, int VEC> struct alignas(sizeof(T) * VEC) MPack { T v[VEC]; };

struct MMArgs {
  int n, B, d, S, n_labels;
  int T[VCT_MM_MAX_MODAL];
  int off[VCT_MM_MAX_MODAL];
  const void* u[VCT_MM_MAX_MODAL];
  const uint8_t* mask[VCT_MM_MAX_MODAL];
  void* du[VCT_MM_MAX_MODAL];
  const float* temp; const float* modal_w; const int32_t* labels;
  void* x0; uint8_t* key_pad; const void* dx; float* d_modal;
};

// temporal row + modal-embedding row (fp32, 4 columns from c): what the reference adds to the features
__device__ __forceinline__ float4 mm_row_add(const MMArgs& a, int row, int c) {
  const int l = a.labels[row];
  const float4 tp = *reinterpret_cast<const float4*>(a.temp + (size_t)row * a.d + c);
  if ((unsigned)l >= (unsigned)a.n_labels) return tp;
  const float4 md = *reinterpret_cast<const float4*>(a.modal_w + (size_t)l * a.d + c);
  return make_float4(tp.x + md.x, tp.y + md.y, tp.z + md.z, tp.w + md.w);
}

template <typename T>
__global__ __launch_bounds__(MM_THREADS) void mm_frontend_fwd_kernel(MMArgs a) {
  constexpr int VEC = MV<T>::VEC;
  using P = MPack<T, VEC>;
  const int b = blockIdx.x, i = blockIdx.y;
  const int Tn = a.T[i], d = a.d, nvec = d / VEC;
  const size_t base = (size_t)b * a.S + a.off[i];
  const T* __restrict__ u = static_cast<const T*>(a.u[i]) + (size_t)b * Tn * d;
  T* __restrict__ x0 = static_cast<T*>(a.x0);
  // frame rows: one (row, column vector) per thread and step
  for (int it = threadIdx.x; it < Tn * nvec; it += MM_THREADS) {
    const int t = it / nvec, vi = it - t * nvec;
    const P uv = *reinterpret_cast<const P*>(u + (size_t)t * d + vi * VEC);
    P o;
#pragma unroll
    for (int q = 0; q < VEC; q += 4) {
      const float4 tm = mm_row_add(a, a.off[i] + 1 + t, vi * VEC + q);
      o.v[q + 0] = from_f<T>(tm.x + to_f<T>(uv.v[q + 0]));
      o.v[q + 1] = from_f<T>(tm.y + to_f<T>(uv.v[q + 1]));
      o.v[q + 2] = from_f<T>(tm.z + to_f<T>(uv.v[q + 2]));
      o.v[q + 3] = from_f<T>(tm.w + to_f<T>(uv.v[q + 3]));
    }
    *reinterpret_cast<P*>(x0 + (base + 1 + t) * d + vi * VEC) = o;
  }
  // aggregation row: the mean over all T_i rows in row order (fp32)
  for (int vi = threadIdx.x; vi < nvec; vi += MM_THREADS) {
    float acc[VEC];
#pragma unroll
    for (int j = 0; j < VEC; j++) acc[j] = 0.0f;
    for (int t = 0; t < Tn; t++) {
      const P uv = *reinterpret_cast<const P*>(u + (size_t)t * d + vi * VEC);
#pragma unroll
      for (int j = 0; j < VEC; j++) acc[j] += to_f<T>(uv.v[j]);
    }
    P o;
#pragma unroll
    for (int q = 0; q < VEC; q += 4) {
      const float4 tm = mm_row_add(a, a.off[i], vi * VEC + q);
      o.v[q + 0] = from_f<T>(tm.x + acc[q + 0] / (float)Tn);
      o.v[q + 1] = from_f<T>(tm.y + acc[q + 1] / (float)Tn);
      o.v[q + 2] = from_f<T>(tm.z + acc[q + 2] / (float)Tn);
      o.v[q + 3] = from_f<T>(tm.w + acc[q + 3] / (float)Tn);
    }
    *reinterpret_cast<P*>(x0 + base * d + vi * VEC) = o;
  }
  if (a.key_pad != nullptr) {
    const uint8_t* mk = a.mask[i];
    for (int t = threadIdx.x; t <= Tn; t += MM_THREADS)
      a.key_pad[base + t] = (t == 0 || mk == nullptr) ? (uint8_t)0 : (uint8_t)(mk[(size_t)b * Tn + t - 1] != 0);
  }
}

template <typename T>
__global__ __launch_bounds__(MM_THREADS) void mm_frontend_bwd_kernel(MMArgs a, int n_groups) {
  constexpr int VEC = MV<T>::VEC;
  using P = MPack<T, VEC>;
  const int d = a.d, nvec = d / VEC;
  const T* __restrict__ dx = static_cast<const T*>(a.dx);
  const int nb_du = a.B * a.n;
  if ((int)blockIdx.x < nb_du) {
    const int b = blockIdx.x / a.n, i = blockIdx.x - b * a.n;
    const int Tn = a.T[i];
    const size_t base = (size_t)b * a.S + a.off[i];
    T* __restrict__ du = static_cast<T*>(a.du[i]) + (size_t)b * Tn * d;
    for (int it = threadIdx.x; it < Tn * nvec; it += MM_THREADS) {
      const int t = it / nvec, vi = it - t * nvec;
      const P g0 = *reinterpret_cast<const P*>(dx + base * d + vi * VEC);
      const P g = *reinterpret_cast<const P*>(dx + (base + 1 + t) * d + vi * VEC);
      P o;
#pragma unroll
      for (int j = 0; j < VEC; j++) o.v[j] = from_f<T>(to_f<T>(g.v[j]) + to_f<T>(g0.v[j]) / (float)Tn);
      *reinterpret_cast<P*>(du + (size_t)t * d + vi * VEC) = o;
    }
    return;
  }
  // modal-embedding gradient of label l, column vectors [g * MM_CV, g * MM_CV + MM_CV)
  __shared__ int s_rows[MM_MAX_ROWS];
  __shared__ int s_cnt;
  __shared__ float s_red[MM_LANES][MM_CV * VEC];
  const int k = blockIdx.x - nb_du;
  const int l = k / n_groups, g = k - l * n_groups;
  if (threadIdx.x == 0) {
    int c = 0;
    for (int s = 0; s < a.S; s++)
      if (a.labels[s] == l) s_rows[c++] = s;
    s_cnt = c;
  }
  __syncthreads();
  const int cnt = s_cnt;
  const int cv = threadIdx.x % MM_CV, lane = threadIdx.x / MM_CV;
  const int vi = g * MM_CV + cv;
  float acc[VEC];
#pragma unroll
  for (int j = 0; j < VEC; j++) acc[j] = 0.0f;
  if (vi < nvec && cnt > 0) {
    const int items = a.B * cnt;
    for (int it = lane; it < items; it += MM_LANES) {
      const int b = it / cnt, s = s_rows[it - b * cnt];
      const P v = *reinterpret_cast<const P*>(dx + ((size_t)b * a.S + s) * d + vi * VEC);
#pragma unroll
      for (int j = 0; j < VEC; j++) acc[j] += to_f<T>(v.v[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < VEC; j++) s_red[lane][cv * VEC + j] = acc[j];
  __syncthreads();
  if (threadIdx.x < MM_CV * VEC) {
    const int col = g * MM_CV * VEC + threadIdx.x;
    if (col < d) {
      float sum = 0.0f;
      for (int r = 0; r < MM_LANES; r++) sum += s_red[r][threadIdx.x];
      a.d_modal[(size_t)l * d + col] = sum;
    }
  }
}

}  // namespace vct
using namespace vct;

static bool mm_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }

// shape / pointer checks shared by both directions; fills the kernel arguments
static int mm_prepare(const vct_mm_frontend_desc* p, bool fwd, MMArgs& a) {
  if (p == nullptr) return VCT_E_ARG;
  if (p->dtype != VCT_F32 && p->dtype != VCT_BF16) return VCT_E_ARG;
  if (p->n < 2 || p->n > VCT_MM_MAX_MODAL || p->B <= 0 || p->d <= 0) return VCT_E_SHAPE;
  if (p->n_labels != p->n && p->n_labels != 2 * p->n) return VCT_E_SHAPE;
  if (p->d % (p->dtype == VCT_BF16 ? 8 : 4)) return VCT_E_ALIGN;
  if (p->labels == nullptr) return VCT_E_ARG;
  a.n = p->n; a.B = p->B; a.d = p->d; a.n_labels = p->n_labels;
  for (int i = 0; i < VCT_MM_MAX_MODAL; i++) {
    a.T[i] = 0; a.off[i] = 0; a.u[i] = nullptr; a.mask[i] = nullptr; a.du[i] = nullptr;
  }
  int S = 0;
  for (int i = 0; i < p->n; i++) {
    if (p->T[i] <= 0) return VCT_E_SHAPE;
    a.T[i] = p->T[i];
    a.off[i] = S;
    S += p->T[i] + 1;
    if (S > MM_MAX_ROWS) return VCT_E_SHAPE;
    if (fwd) {
      if (p->u[i] == nullptr) return VCT_E_ARG;
      if (!mm_aligned(p->u[i])) return VCT_E_ALIGN;
      a.u[i] = p->u[i];
      a.mask[i] = p->mask[i];
    } else {
      if (p->du[i] == nullptr) return VCT_E_ARG;
      if (!mm_aligned(p->du[i])) return VCT_E_ALIGN;
      a.du[i] = p->du[i];
    }
  }
  a.S = S;
  a.labels = p->labels;
  a.temp = p->temp; a.modal_w = p->modal_w; a.x0 = p->x0; a.key_pad = p->key_pad;
  a.dx = p->dx; a.d_modal = p->d_modal;
  if (fwd) {
    if (!p->temp || !p->modal_w || !p->x0) return VCT_E_ARG;
    if (!mm_aligned(p->temp) || !mm_aligned(p->modal_w) || !mm_aligned(p->x0)) return VCT_E_ALIGN;
  } else {
    if (!p->dx || !p->d_modal) return VCT_E_ARG;
    if (!mm_aligned(p->dx)) return VCT_E_ALIGN;
  }
  return VCT_OK;
}

extern "C" int vct_mm_frontend_fwd(const vct_mm_frontend_desc* p, void* stream) {
  MMArgs a;
  const int rc = mm_prepare(p, true, a);
  if (rc != VCT_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (p->dtype == VCT_BF16)
    vct::launch((mm_frontend_fwd_kernel<bf16_t>), dim3(a.B, a.n), dim3(MM_THREADS), 0, st, a);
  else
    vct::launch((mm_frontend_fwd_kernel<float>), dim3(a.B, a.n), dim3(MM_THREADS), 0, st, a);
  VCT_CHECK_LAUNCH();
  return VCT_OK;
}

extern "C" int vct_mm_frontend_bwd(const vct_mm_frontend_desc* p, void* stream) {
  MMArgs a;
  const int rc = mm_prepare(p, false, a);
  if (rc != VCT_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int vec = p->dtype == VCT_BF16 ? 8 : 4;
  const int n_groups = (a.d / vec + MM_CV - 1) / MM_CV;
  const dim3 grid(a.B * a.n + a.n_labels * n_groups);
  if (p->dtype == VCT_BF16)
    vct::launch((mm_frontend_bwd_kernel<bf16_t>), grid, dim3(MM_THREADS), 0, st, a, n_groups);
  else
    vct::launch((mm_frontend_bwd_kernel<float>), grid, dim3(MM_THREADS), 0, st, a, n_groups);
  VCT_CHECK_LAUNCH();
  return VCT_OK;
}
