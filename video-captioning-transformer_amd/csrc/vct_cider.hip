// The self-critical reward on gfx950: CIDEr-D of sampled token ids against device-resident reference tables (vct_cider_d) and
// the advantages in the layout of vct_wce_loss's seq_w (vct_scst_advantages).  Table layout, key hash and semantics:
// include/vct_hip.h.  Everything behind the integer counts is fp64 and every sum runs serially in the order rewards.CiderD sums
// on the host (first occurrence of the candidate's n-grams), without contraction into fused multiply-adds, so the two differ by
// the exponential's last bit at most.
#include "vct_common.h"
#include <math.h>

namespace vct {

struct CiderKey { int w[4]; };

__device__ __forceinline__ uint32_t cider_hash(const CiderKey& k) {
  uint32_t h = 0x811C9DC5u;
#pragma unroll
  for (int j = 0; j < 4; j++) h = (h ^ (uint32_t)k.w[j]) * 0x01000193u;
  return hash32(h);
}
__device__ __forceinline__ CiderKey cider_load_key(const int32_t* keys, int64_t i) {
  const int4 v = *reinterpret_cast<const int4*>(keys + 4 * i);
  CiderKey k;
  k.w[0] = v.x; k.w[1] = v.y; k.w[2] = v.z; k.w[3] = v.w;
  return k;
}
// lexicographic compare as signed words: < 0, 0, > 0
__device__ __forceinline__ int cider_cmp(const CiderKey& a, const CiderKey& b) {
#pragma unroll
  for (int j = 0; j < 4; j++)
    if (a.w[j] != b.w[j]) return a.w[j] < b.w[j] ? -1 : 1;
  return 0;
}

// One workgroup per candidate; wave k holds the n-gram instances of order k + 1, lane p the one that starts at token p.
// EVAL (vct_cider_d_eval): the candidate is cut BEFORE its first end token and the un-rounded fp64 score is written as well.
template <bool EVAL>
__global__ __launch_bounds__(256) void cider_d_kernel(const vct_cider_desc d, double* score) {
#pragma clang fp contract(off)
  __shared__ int tok[VCT_CIDER_MAX_LEN];
  __shared__ double term[4 * VCT_CIDER_MAX_LEN];
  __shared__ double cnorm[4], sk[4];
  __shared__ int s_len;
  const int c = blockIdx.x, b = c / d.N, s = c - b * d.N, tid = threadIdx.x;
  const int L = d.L;
  if (tid < 64) {
    int64_t v = -1;
    if (tid < L) v = d.ids[(int64_t)b * d.stride_b + (int64_t)s * d.stride_n + (int64_t)(1 + tid) * d.stride_l];
    const unsigned long long ends = __ballot(tid < L && v == d.end_id);
    tok[tid] = (v < 0 || v > 0x7fffffffLL) ? -2 : (int)v;                 // -2: a word no table key holds (theirs are >= 0 or -1)
    if (tid == 0) s_len = ends ? __ffsll(ends) - (EVAL ? 1 : 0) : L;     // the first end token is kept (reward) / dropped (EVAL)
  }
  __syncthreads();
  const int lc = s_len, k = tid >> 6, p = tid & 63;
  const bool inst = k < d.n && p + k < lc;
  CiderKey key;
#pragma unroll
  for (int j = 0; j < 4; j++) key.w[j] = -1;
  int tf = 0;
  bool first = inst;
  if (inst) {
#pragma unroll
    for (int j = 0; j < 4; j++)
      if (j <= k) key.w[j] = tok[p + j];
    const int cnt = lc - k;                                              // instances of this order: starts 0 .. cnt - 1
    for (int q = 0; q < cnt; q++) {
      bool eq = true;
#pragma unroll
      for (int j = 0; j < 4; j++)
        if (j <= k) eq = eq && (tok[q + j] == key.w[j]);                 // q + j <= lc - 1
      tf += eq ? 1 : 0;
      if (eq && q < p) first = false;
    }
  }
  // the first instance of every unique n-gram carries it: idf from the corpus table (bounded probe), c_w = tf * idf
  double cw = 0.0;
  if (first) {
    double idf = d.log_nvid;
    const uint32_t msk = (uint32_t)d.table_cap - 1u;
    uint32_t slot = cider_hash(key) & msk;
    for (int i = 0; i < d.table_cap; i++) {
      const CiderKey t = cider_load_key(d.table_keys, slot);
      if (t.w[0] == -1) break;
      if (cider_cmp(t, key) == 0) { idf = d.table_idf[slot]; break; }
      slot = (slot + 1u) & msk;
    }
    cw = (double)tf * idf;
  }
  term[tid] = cw * cw;
  __syncthreads();
  if (tid < 4) {
    double sq = 0.0;
    for (int q = 0; q < 64; q++) sq += term[tid * 64 + q];
    cnorm[tid] = sqrt(sq);
  }
  __syncthreads();
  const int row = d.vid_rows[b];
  int r0 = 0, r1 = 0;
  if (row >= 0 && row < d.n_videos) { r0 = d.vid_ref_ptr[row]; r1 = d.vid_ref_ptr[row + 1]; }
  double total = 0.0;
  for (int r = r0; r < r1; r++) {                                        // (uniform over the workgroup: r0, r1 depend on b only)
    double t = 0.0;
    if (first) {
      int lo = d.ref_ent_ptr[r], hi = d.ref_ent_ptr[r + 1];              // bisection over the reference's sorted keys
      while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        const int cm = cider_cmp(cider_load_key(d.ent_keys, mid), key);
        if (cm == 0) {
          const double rw = d.ent_w[mid];
          t = fmin(cw, rw) * rw;
          break;
        }
        if (cm < 0) lo = mid + 1; else hi = mid;
      }
    }
    term[tid] = t;
    __syncthreads();
    if (tid < 4) {
      double sum = 0.0;
      for (int q = 0; q < 64; q++) sum += term[tid * 64 + q];
      sk[tid] = sum;
    }
    __syncthreads();
    if (tid == 0) {
      const double dl = (double)(lc - d.ref_len[r]);
      const double pen = exp(-(dl * dl) / d.two_sigma_sq);
      for (int o = 0; o < d.n; o++) {
        const double rn = d.ref_norm[4 * (int64_t)r + o];
        if (cnorm[o] == 0.0 || rn == 0.0) continue;
        total += pen * sk[o] / (cnorm[o] * rn);
      }
    }
  }
  if (tid == 0) {
    if (EVAL) {
      const double sc = (r1 > r0) ? 10.0 * total / (double)(d.n * (r1 - r0)) : 0.0;
      score[c] = sc;
      if (d.reward != nullptr) d.reward[c] = (float)sc;
    } else {
      d.reward[c] = (r1 > r0) ? (float)(10.0 * total / (double)(d.n * (r1 - r0))) : 0.0f;
    }
  }
}

// ONE workgroup: thread t takes the videos t, t + 1024, ...; the two means are a fixed-order tree over the threads' fp64 partials.
__global__ __launch_bounds__(1024) void scst_advantages_kernel(int B, int N, const float* rewards, const float* baseline, float* adv,
                                                               float* base_out, float* means) {
#pragma clang fp contract(off)
  __shared__ double red_r[1024], red_b[1024];
  const int tid = threadIdx.x;
  double part_r = 0.0, part_b = 0.0;
  for (int b = tid; b < B; b += 1024) {
    const float* r = rewards + (size_t)b * N;
    double sum = 0.0;
    for (int n = 0; n < N; n++) sum += (double)r[n];
    part_r += sum;
    if (baseline != nullptr) {
      const float bs = baseline[b];
      for (int n = 0; n < N; n++) adv[(size_t)b * N + n] = (float)((double)r[n] - (double)bs);
      base_out[b] = bs;
      part_b += (double)bs;
    } else {
      for (int n = 0; n < N; n++) {
        const double rn = (double)r[n];                                  // (read before the store: adv may alias rewards)
        adv[(size_t)b * N + n] = (float)(rn - (sum - rn) / (double)(N - 1));
      }
      const float bs = (float)(sum / (double)N);
      base_out[b] = bs;
      part_b += (double)bs;
    }
  }
  red_r[tid] = part_r;
  red_b[tid] = part_b;
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if (tid < o) { red_r[tid] += red_r[tid + o]; red_b[tid] += red_b[tid + o]; }
    __syncthreads();
  }
  if (tid == 0) {
    means[0] = (float)(red_r[0] / ((double)B * (double)N));
    means[1] = (float)(red_b[0] / (double)B);
  }
}

}  // namespace vct

using namespace vct;

// the refusals vct_cider_d and vct_cider_d_eval share, in vct_cider_d's order (reward is optional for the evaluation score)
static int cider_check(const vct_cider_desc* d, bool need_reward) {
  if (!d) return VCT_E_ARG;
  if (d->B < 1 || d->N < 1 || d->L < 0 || d->L > VCT_CIDER_MAX_LEN || d->n < 1 || d->n > VCT_CIDER_MAX_ORDER) return VCT_E_SHAPE;
  if (d->table_cap < 1 || (d->table_cap & (d->table_cap - 1)) || d->n_videos < 0) return VCT_E_SHAPE;
  if ((int64_t)d->B * d->N > 0x7fffffffLL) return VCT_E_SHAPE;
  if (!d->ids || !d->vid_rows || !d->table_keys || !d->table_idf || !d->vid_ref_ptr || !d->ref_len || !d->ref_norm || !d->ref_ent_ptr ||
      !d->ent_keys || !d->ent_w || (need_reward && !d->reward))
    return VCT_E_ARG;
  if (!(d->two_sigma_sq > 0.0)) return VCT_E_ARG;
  if (((uintptr_t)d->table_idf & 7) || ((uintptr_t)d->ref_norm & 7) || ((uintptr_t)d->ent_w & 7)) return VCT_E_ALIGN;
  if (((uintptr_t)d->table_keys & 15) || ((uintptr_t)d->ent_keys & 15)) return VCT_E_ALIGN;
  if (((uintptr_t)d->ids & 7) || ((uintptr_t)d->vid_rows & 3) || ((uintptr_t)d->reward & 3)) return VCT_E_ALIGN;
  return VCT_OK;
}

extern "C" int vct_cider_d(const vct_cider_desc* d, void* stream) {
  const int rc = cider_check(d, true);
  if (rc != VCT_OK) return rc;
  vct::launch(cider_d_kernel<false>, dim3((unsigned)(d->B * d->N)), dim3(256), 0, (hipStream_t)stream, *d, (double*)nullptr);
  VCT_CHECK_LAUNCH();
  return VCT_OK;
}

extern "C" int vct_cider_d_eval(const vct_cider_desc* d, double* score, void* stream) {
  const int rc = cider_check(d, false);
  if (rc != VCT_OK) return rc;
  if (!score) return VCT_E_ARG;
  if ((uintptr_t)score & 7) return VCT_E_ALIGN;
  vct::launch(cider_d_kernel<true>, dim3((unsigned)(d->B * d->N)), dim3(256), 0, (hipStream_t)stream, *d, score);
  VCT_CHECK_LAUNCH();
  return VCT_OK;
}

extern "C" int vct_scst_advantages(int B, int N, const float* rewards, const float* baseline, float* adv, float* base_out,
                                   float* means, void* stream) {
  if (!rewards || !adv || !base_out || !means) return VCT_E_ARG;
  if (B < 1 || N < 1 || (!baseline && N < 2)) return VCT_E_SHAPE;
  vct::launch(scst_advantages_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, B, N, rewards, baseline, adv, base_out, means);
  VCT_CHECK_LAUNCH();
  return VCT_OK;
}
