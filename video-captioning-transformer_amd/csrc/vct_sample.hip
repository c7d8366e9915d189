// Sampled token selection for the KV-cached decode step on gfx950: temperature, top-k and nucleus (top-p within the top k).
//
// replaces: nothing in the reference (it decodes greedily, MMT4Caption.py:146-184); the semantics are the project's
// (include/vct_hip.h, vct_sample_select; decode.sample_decode_ids).  Every setting is read from a 16-byte control block in
// device memory, so the captured per-position graphs serve every seed / temperature / k / p; grid and workspace are sized for
// the largest k (64).
//
// vct_sample_select, two launches (vct_beam_select's shape: the partials reach stage 2 through the kernel boundary, so no
// inter-workgroup hand-off inside a launch):
//   stage 1  grid (rows, V chunks), 256 threads, one 16-byte load per thread.  top_k == 0: the chunk's max and its sum of
//            exp(z - chunk max).  top_k >= 1: the chunk's top k (logit, column), by k rounds of a workgroup arg-max.
//            Rows that had ended before the step return at once.
//   stage 2  one workgroup per row.  top_k == 0: row max and W from the chunk partials in chunk order, the chunk that holds
//            u * W, then an inclusive workgroup scan of exp(z - m) over that chunk's elements (re-read: 4 KB) and the first
//            element whose running sum exceeds what is left of u * W.  top_k >= 1: wave 0 merges the sorted chunk lists (one
//            list head per lane, k rounds of a wave arg-max), lane r ends up with the rank-r candidate; max, inclusive scan,
//            nucleus cut and draw are wave operations over those <= 64 lanes.
// Reductions and scans have a fixed order (shuffle trees, then a sequential pass over the waves / chunks): no floating-point
// atomics, a second call is bit-identical.  Integer atomics only for the end bookkeeping, as vct_greedy_select.
// The tie rule, the chunk scan of stage 1, the arg-max reductions and the end bookkeeping are vct_select_core.h's, shared with
// vct_select.hip and vct_beam.hip.
#include "vct_select_core.h"

namespace vct {

constexpr int SMP_THREADS = SEL_THREADS;
constexpr int SMP_WAVES = SEL_WAVES;
constexpr int SMP_KMAX = 64;                // one candidate per lane of the merging wave
constexpr int SMP_CHMAX = 64;               // one chunk list per lane of the merging wave
constexpr uint32_t SMP_SITE = 997u;         // the counter hash's site (engine/stack.py, SAMPLE_SITE)

// inclusive prefix sum over the 64 lanes (Hillis-Steele: a fixed order)
__device__ __forceinline__ float smp_wave_scan(float v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float up = __shfl_up(v, o);
    if (lane >= o) v += up;
  }
  return v;
}

__device__ __forceinline__ int smp_clamp_k(int k, int V) { return k < 0 ? 0 : (k > SMP_KMAX ? min(SMP_KMAX, V) : min(k, V)); }

template <typename T>
__global__ __launch_bounds__(SMP_THREADS) void sample_partial_kernel(int V, const T* __restrict__ x, int64_t ldx, bool vec_ok,
                                                                     const uint8_t* __restrict__ ended,
                                                                     const vct_sample_ctl* __restrict__ ctl, float* __restrict__ pmax,
                                                                     float* __restrict__ psum, float* __restrict__ ptv,
                                                                     int* __restrict__ pti) {
  constexpr int VEC = 16 / (int)sizeof(T);
  __shared__ float s_v[2][SMP_WAVES];
  __shared__ int s_i[2][SMP_WAVES];
  __shared__ float s_sum[SMP_WAVES];
  const int row = blockIdx.x, chunk = blockIdx.y, CH = gridDim.y;
  if (ended[row]) return;                    // (the whole workgroup: stage 2 reads no partial of such a row)
  const int K = smp_clamp_k(ctl->top_k, V);
  const float inv_temp = ctl->inv_temp;
  float e[VEC];
  int id[VEC];
  sel_chunk_load<T, VEC>(x + (size_t)row * ldx, (chunk * SMP_THREADS + threadIdx.x) * VEC, V, vec_ok, e, id);
  float hv, mv;
  int hi, mi;
  sel_head(e, id, hv, hi);
  mv = hv; mi = hi;
  sel_block_best<SMP_WAVES>(mv, mi, s_v, s_i, 0);
  const size_t pc = (size_t)row * CH + chunk;
  if (K == 0) {
    // the chunk's max logit and its sum of exp(z - z_max), z = x * inv_temp (rounded as stage 2 rounds it)
    const float se = sel_chunk_expsum(e, id, inv_temp, mv * inv_temp, s_sum);
    if (threadIdx.x == 0) { pmax[pc] = mv; psum[pc] = se; }
    return;
  }
  sel_chunk_topk(K, e, id, hv, hi, mv, mi, s_v, s_i, ptv, pti, pc, SMP_KMAX);
}

// the uniform of (seed, step t, row r): 24 bits, stateless
__device__ __forceinline__ float smp_uniform(uint32_t seed, int t, int rows, int r) {
  const uint32_t key = (seed * 0x9E3779B1u) ^ (SMP_SITE * 0x85EBCA77u + 0x165667B1u);
  const uint32_t k = hash32(key);
  const uint32_t idx = (uint32_t)t * (uint32_t)rows + (uint32_t)r;
  const uint32_t h = hash32(k + idx * 0x9E3779B1u);
  return (float)(h >> 8) * (1.0f / 16777216.0f);
}

template <typename T>
__global__ __launch_bounds__(SMP_THREADS) void sample_draw_kernel(int V, int CH, const T* __restrict__ x, int64_t ldx, bool vec_ok,
                                                                  const vct_sample_ctl* __restrict__ ctl, const float* __restrict__ pmax,
                                                                  const float* __restrict__ psum, const float* __restrict__ ptv,
                                                                  const int* __restrict__ pti, int64_t* __restrict__ out,
                                                                  int64_t out_stride, int64_t end_id, int64_t pad_id,
                                                                  uint8_t* __restrict__ ended, int32_t* ended_count,
                                                                  unsigned long long* all_ended_at, float* __restrict__ step_logp,
                                                                  float* __restrict__ seq_logp, int t) {
  constexpr int VEC = 16 / (int)sizeof(T);
  constexpr int CHUNK = SMP_THREADS * VEC;
  __shared__ float s_cv[SMP_CHMAX * SMP_KMAX];      // the chunk lists of the row (top_k >= 1): CH * K entries
  __shared__ int s_ci[SMP_CHMAX * SMP_KMAX];
  __shared__ float s_tot[SMP_WAVES];
  __shared__ int s_first[SMP_WAVES];
  const int row = blockIdx.x, rows = gridDim.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (ended[row]) {
    if (threadIdx.x == 0) { out[(size_t)row * out_stride] = pad_id; step_logp[row] = 0.0f; }
    return;
  }
  const int K = smp_clamp_k(ctl->top_k, V);
  const float inv_temp = ctl->inv_temp, top_p = ctl->top_p;
  const float u01 = smp_uniform(ctl->seed, t, rows, row);
  const T* r = x + (size_t)row * ldx;
  int tok = SEL_NONE;
  float logp = 0.0f;
  if (K == 0) {
    // row max, W and the chunk that holds u * W: every thread walks the <= 64 chunk partials in chunk order
    const size_t base = (size_t)row * CH;
    float mx = -INFINITY;
    for (int c = 0; c < CH; c++) mx = fmaxf(mx, pmax[base + c]);
    const float m = mx * inv_temp;
    float W = 0.0f;
    for (int c = 0; c < CH; c++) W += psum[base + c] * expf(pmax[base + c] * inv_temp - m);
    const float target = u01 * W;
    int cs = CH - 1;
    float run = 0.0f, before = 0.0f;
    for (int c = 0; c < CH; c++) {
      before = run;
      run += psum[base + c] * expf(pmax[base + c] * inv_temp - m);
      if (run > target) { cs = c; break; }
    }
    const float rem = target - before;
    // inclusive scan of exp(z - m) over the chunk's elements in index order
    float e[VEC];
    int id[VEC];
    sel_chunk_load<T, VEC>(r, cs * CHUNK + threadIdx.x * VEC, V, vec_ok, e, id);
    float pre[VEC];
    float tt = 0.0f;
#pragma unroll
    for (int q = 0; q < VEC; q++) {
      tt += (id[q] != SEL_NONE) ? expf(e[q] * inv_temp - m) : 0.0f;
      pre[q] = tt;
    }
    const float inc = smp_wave_scan(tt, lane);
    if (lane == 63) s_tot[wv] = inc;
    __syncthreads();
    float off = inc - tt;
    for (int w = 0; w < wv; w++) off += s_tot[w];
    int first = SEL_NONE;
#pragma unroll
    for (int q = VEC - 1; q >= 0; q--)
      if (id[q] != SEL_NONE && off + pre[q] > rem) first = id[q];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) first = min(first, __shfl_xor(first, o));
    if (lane == 0) s_first[wv] = first;
    __syncthreads();
    if (threadIdx.x != 0) return;
    first = s_first[0];
#pragma unroll
    for (int w = 1; w < SMP_WAVES; w++) first = min(first, s_first[w]);
    tok = first != SEL_NONE ? first : min(V, (cs + 1) * CHUNK) - 1;       // rounding left none: the chunk's last element
    logp = to_f<T>(r[tok]) * inv_temp - m - logf(W);
  } else {
    const size_t base = (size_t)row * CH * SMP_KMAX;
    for (int i = threadIdx.x; i < CH * K; i += SMP_THREADS) {
      const int c = i / K, j = i - c * K;
      s_cv[i] = ptv[base + (size_t)c * SMP_KMAX + j];
      s_ci[i] = pti[base + (size_t)c * SMP_KMAX + j];
    }
    __syncthreads();
    if (wv != 0) return;
    // K-way merge of the sorted chunk lists: lane c holds the head of chunk c's list, lane r keeps the rank-r winner
    int h = 0;
    float cv = lane < CH ? s_cv[lane * K] : -INFINITY;
    int ci = lane < CH ? s_ci[lane * K] : SEL_NONE;
    float myv = -INFINITY;
    int myi = SEL_NONE;
    for (int k = 0; k < K; k++) {
      float bv = cv;
      int bi = ci;
      sel_wave_best(bv, bi);
      if (lane == k) { myv = bv; myi = bi; }
      if (bi == ci && bi != SEL_NONE) {
        h++;
        cv = h < K ? s_cv[lane * K + h] : -INFINITY;
        ci = h < K ? s_ci[lane * K + h] : SEL_NONE;
      }
    }
    const bool cand = lane < K && myi != SEL_NONE;
    const float z = cand ? myv * inv_temp : -INFINITY;
    const float m = wave_max(z);
    const float w = cand ? expf(z - m) : 0.0f;
    const float inc = smp_wave_scan(w, lane);
    int keep = K;
    if (top_p < 1.0f) {                       // the shortest rank-order prefix that reaches top_p of the candidates' sum
      const float thr = top_p * __shfl(inc, K - 1);
      const unsigned long long reach = __ballot(cand && inc >= thr);
      if (reach) keep = __ffsll(reach);
    }
    const float W = __shfl(inc, keep - 1);
    const unsigned long long hit = __ballot(cand && lane < keep && inc > u01 * W);
    const int sel = hit ? __ffsll(hit) - 1 : keep - 1;
    tok = __shfl(myi, sel);
    logp = __shfl(z, sel) - m - logf(W);
    if (lane != 0) return;
  }
  // one thread per row from here
  if (tok == SEL_NONE || tok < 0 || tok >= V) tok = 0;      // (only a row without a finite logit gets here)
  out[(size_t)row * out_stride] = tok;
  step_logp[row] = logp;
  seq_logp[row] += logp;
  if ((int64_t)tok == end_id) sel_mark_ended(&ended[row], 1, ended_count, rows, all_ended_at, t);
}

}  // namespace vct
using namespace vct;

extern "C" int64_t vct_sample_select_workspace_bytes(int dtype, int rows, int V) {
  if (!dt_ok(dtype) || rows < 1 || V < 1) return 0;
  return (int64_t)rows * sel_chunks(dtype, V) * (2 + 2 * SMP_KMAX) * 4;
}

template <typename T>
static void sample_launch(const vct_sample_select_desc* d, int CH, hipStream_t st) {
  const int rows = d->rows, V = d->V;
  const size_t MC = (size_t)rows * (size_t)CH;
  float* pmax = (float*)d->workspace;
  float* psum = pmax + MC;
  float* ptv = psum + MC;
  int* pti = (int*)(ptv + MC * SMP_KMAX);
  const bool vec_ok = (((uintptr_t)d->x) & 15) == 0 && (((size_t)d->ldx * sizeof(T)) & 15) == 0;
  unsigned long long* at = reinterpret_cast<unsigned long long*>(d->all_ended_at);
  vct::launch((sample_partial_kernel<T>), dim3(rows, (unsigned)CH), dim3(SMP_THREADS), 0, st, V, (const T*)d->x, d->ldx, vec_ok,
              (const uint8_t*)d->ended, d->ctl, pmax, psum, ptv, pti);
  vct::launch((sample_draw_kernel<T>), dim3(rows), dim3(SMP_THREADS), 0, st, V, CH, (const T*)d->x, d->ldx, vec_ok, d->ctl,
              (const float*)pmax, (const float*)psum, (const float*)ptv, (const int*)pti, d->out, d->out_stride, d->end_id, d->pad_id,
              d->ended, d->ended_count, at, d->step_logp, d->seq_logp, (int)d->t);
}

extern "C" int vct_sample_select(const vct_sample_select_desc* d, void* stream) {
  if (!d || !dt_ok(d->dtype) || !d->x || !d->out || !d->ended || !d->ended_count || !d->all_ended_at || !d->step_logp ||
      !d->seq_logp || !d->ctl || !d->workspace)
    return VCT_E_ARG;
  const int rows = d->rows, V = d->V;
  if (rows < 1 || V < 1 || d->ldx < V || d->out_stride <= 0 || d->t < 0) return VCT_E_SHAPE;
  const int64_t CH = sel_chunks(d->dtype, V);
  if (CH > SMP_CHMAX) return VCT_E_SHAPE;                         // one chunk list per lane of the merging wave
  if ((((uintptr_t)d->ctl) & 15) != 0 || (((uintptr_t)d->workspace) & 15) != 0) return VCT_E_ALIGN;
  if (d->workspace_bytes < vct_sample_select_workspace_bytes(d->dtype, rows, V)) return VCT_E_WORKSPACE;
  if (d->dtype == VCT_BF16) sample_launch<bf16_t>(d, (int)CH, (hipStream_t)stream);
  else sample_launch<float>(d, (int)CH, (hipStream_t)stream);
  VCT_CHECK_LAUNCH();
  return VCT_OK;
}
