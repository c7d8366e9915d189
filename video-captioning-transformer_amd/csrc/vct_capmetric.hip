// Caption metrics for evaluation on gfx950: the per-caption integer statistics of BLEU-1..4 and ROUGE-L (vct_capmetric_counts) and
// the corpus-level fold of those rows and the per-caption CIDEr values into the eight reported numbers (vct_capmetric_finish).
// Semantics, table layout and refusals: include/vct_hip.h; the CIDEr value itself is vct_cider_d_eval (vct_cider.hip).
// Every integer is exact; the few fp64 operations run without contraction into fused multiply-adds, as metrics.CaptionMetrics
// computes them on the host.
#include "vct_common.h"
#include <math.h>

namespace vct {

// One workgroup per caption.  Clipped n-gram counts: wave k holds the instances of order k + 1, lane p the one that starts at token
// p (the layout of cider_d_kernel); the first instance of every distinct n-gram counts itself in every reference, straight on the
// token arrays.  LCS: wave k takes the references r0 + k, r0 + k + 4, ..., one 64-bit row word per wave.
__global__ __launch_bounds__(256) void capmetric_counts_kernel(const vct_capmetric_desc d) {
#pragma clang fp contract(off)
  __shared__ int tok[VCT_CIDER_MAX_LEN];
  __shared__ int s_len;
  __shared__ int w_corr[4], w_lcs[4], w_num[4], w_den[4];
  const int c = blockIdx.x, tid = threadIdx.x, L = d.L;
  if (tid < 64) {
    int64_t v = -1;
    if (tid < L) v = d.ids[(int64_t)c * d.stride_c + (int64_t)(1 + tid) * d.stride_l];
    const unsigned long long ends = __ballot(tid < L && v == d.end_id);
    tok[tid] = (v < 0 || v > 0x7fffffffLL) ? -2 : (int)v;                 // -2: a word no reference holds (theirs are >= 0)
    if (tid == 0) s_len = ends ? __ffsll(ends) - 1 : L;                  // the first end token is dropped
  }
  __syncthreads();
  const int lc = s_len, k = tid >> 6, p = tid & 63;
  const int row = d.vid_rows[c];
  int r0 = 0, r1 = 0;
  if (row >= 0 && row < d.n_videos) { r0 = d.vid_ref_ptr[row]; r1 = d.vid_ref_ptr[row + 1]; }

  // ---- clipped counts of order k + 1 ----
  const bool inst = p + k < lc;
  int key[4] = {-1, -1, -1, -1};
  int tf = 0;
  bool first = inst;
  if (inst) {
#pragma unroll
    for (int j = 0; j < 4; j++)
      if (j <= k) key[j] = tok[p + j];
    const int cnt = lc - k;                                              // instances of this order: starts 0 .. cnt - 1
    for (int q = 0; q < cnt; q++) {
      bool eq = true;
#pragma unroll
      for (int j = 0; j < 4; j++)
        if (j <= k) eq = eq && (tok[q + j] == key[j]);                   // q + j <= lc - 1
      tf += eq ? 1 : 0;
      if (eq && q < p) first = false;
    }
  }
  int clip = 0;
  if (first) {
    int best = 0;
    for (int r = r0; r < r1 && best < tf; r++) {                         // (more than tf occurrences clip to tf anyway)
      const int t0 = d.ref_tok_ptr[r];
      const int cnt = d.ref_tok_ptr[r + 1] - t0 - k;                     // n-gram starts in this reference
      const int32_t* rt = d.ref_tok + t0;
      int occ = 0;
      for (int q = 0; q < cnt; q++) {
        bool eq = true;
#pragma unroll
        for (int j = 0; j < 4; j++)
          if (j <= k) eq = eq && (rt[q + j] == key[j]);                  // q + j <= len_r - 1
        occ += eq ? 1 : 0;
      }
      best = occ > best ? occ : best;
    }
    clip = tf < best ? tf : best;
  }
  for (int o = 32; o > 0; o >>= 1) clip += __shfl_down(clip, o);         // integers: any order is exact
  if (p == 0) w_corr[k] = clip;

  // ---- LCS against the references r0 + k, r0 + k + 4, ... (r, its length and V are uniform over the wave) ----
  const unsigned long long low = lc >= 64 ? ~0ull : ((1ull << lc) - 1ull);
  const int mine = p < lc ? tok[p] : -2;
  int lcs_max = 0, bn = 0, bd = 1;                                       // the best LCS_r / len_r so far, as a fraction
  for (int r = r0 + k; r < r1; r += 4) {
    const int t0 = d.ref_tok_ptr[r], lr = d.ref_tok_ptr[r + 1] - t0;
    unsigned long long V = ~0ull;
    for (int i = 0; i < lr; i++) {
      const int t = d.ref_tok[t0 + i];
      const unsigned long long M = __ballot(p < lc && mine == t);
      const unsigned long long U = V & M;
      V = (V + U) | (V - U);
    }
    const int lcs = __popcll(~V & low);
    lcs_max = lcs > lcs_max ? lcs : lcs_max;
    if (lr > 0 && (long long)lcs * bd > (long long)bn * lr) { bn = lcs; bd = lr; }
  }
  if (p == 0) { w_lcs[k] = lcs_max; w_num[k] = bn; w_den[k] = bd; }
  __syncthreads();

  if (tid == 0) {
    int32_t* o = d.counts + (int64_t)VCT_CAPMETRIC_COUNT_COLS * c;
    double* ro = d.rouge + 3 * (int64_t)c;
    if (r1 <= r0) {                                                      // no references: an all-zero row
      for (int j = 0; j < VCT_CAPMETRIC_COUNT_COLS; j++) o[j] = 0;
      ro[0] = ro[1] = ro[2] = 0.0;
      return;
    }
    int reflen = 0, bdiff = 0x7fffffff;
    for (int r = r0; r < r1; r++) {
      const int lr = d.ref_tok_ptr[r + 1] - d.ref_tok_ptr[r];
      const int df = lr > lc ? lr - lc : lc - lr;
      if (df < bdiff || (df == bdiff && lr < reflen)) { bdiff = df; reflen = lr; }
    }
    for (int w = 1; w < 4; w++) {
      lcs_max = w_lcs[w] > lcs_max ? w_lcs[w] : lcs_max;
      if ((long long)w_num[w] * bd > (long long)bn * w_den[w]) { bn = w_num[w]; bd = w_den[w]; }
    }
    o[0] = lc;
    o[1] = reflen;
    for (int j = 0; j < 4; j++) {
      o[2 + j] = w_corr[j];
      o[6 + j] = lc - j > 0 ? lc - j : 0;
    }
    o[10] = lcs_max;
    o[11] = 0;
    const double prec = lc > 0 ? (double)lcs_max / (double)lc : 0.0;
    const double rec = (double)bn / (double)bd;
    double f = 0.0;
    if (prec != 0.0 && rec != 0.0) f = (1.0 + d.beta_sq) * prec * rec / (rec + d.beta_sq * prec);
    ro[0] = prec;
    ro[1] = rec;
    ro[2] = f;
  }
}

#define CAPMETRIC_FINISH_THREADS 256

// ONE workgroup: thread t takes the rows t, t + 256, ...; the sums are a fixed-order tree over the threads' partials.
__global__ __launch_bounds__(CAPMETRIC_FINISH_THREADS) void capmetric_finish_kernel(int C, const int32_t* counts, const double* rouge,
                                                                                   const double* cider, double* out) {
#pragma clang fp contract(off)
  __shared__ long long red_i[10][CAPMETRIC_FINISH_THREADS];
  __shared__ double red_f[2][CAPMETRIC_FINISH_THREADS];
  const int tid = threadIdx.x;
  long long pi[10];
  for (int j = 0; j < 10; j++) pi[j] = 0;
  double pf = 0.0, pc = 0.0;
  for (int c = tid; c < C; c += CAPMETRIC_FINISH_THREADS) {
    const int32_t* r = counts + (int64_t)VCT_CAPMETRIC_COUNT_COLS * c;
    for (int j = 0; j < 10; j++) pi[j] += (long long)r[j];
    pf += rouge[3 * (int64_t)c + 2];
    if (cider != nullptr) pc += cider[c];
  }
  for (int j = 0; j < 10; j++) red_i[j][tid] = pi[j];
  red_f[0][tid] = pf;
  red_f[1][tid] = pc;
  __syncthreads();
  for (int o = CAPMETRIC_FINISH_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) {
      for (int j = 0; j < 10; j++) red_i[j][tid] += red_i[j][tid + o];
      red_f[0][tid] += red_f[0][tid + o];
      red_f[1][tid] += red_f[1][tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const double tiny = 1e-15, small = 1e-9;
    const double testlen = (double)red_i[0][0], reflen = (double)red_i[1][0];
    double bleu[4];
    double p = 1.0;
    for (int k = 0; k < 4; k++) {
      p *= ((double)red_i[2 + k][0] + tiny) / ((double)red_i[6 + k][0] + small);
      bleu[k] = pow(p, 1.0 / (double)(k + 1));
    }
    const double ratio = (testlen + tiny) / (reflen + small);
    if (ratio < 1.0) {
      const double bp = exp(1.0 - 1.0 / ratio);
      for (int k = 0; k < 4; k++) bleu[k] *= bp;
    }
    const double rl = red_f[0][0] / (double)C;
    const double cd = cider != nullptr ? red_f[1][0] / (double)C : 0.0;
    for (int k = 0; k < 4; k++) out[k] = bleu[k];
    out[4] = rl;
    out[5] = cd;
    out[6] = bleu[3] + rl + cd;
    out[7] = (double)C;
  }
}

}  // namespace vct

using namespace vct;

extern "C" int vct_capmetric_counts(const vct_capmetric_desc* d, void* stream) {
  if (!d) return VCT_E_ARG;
  if (d->C < 1 || d->L < 0 || d->L > VCT_CIDER_MAX_LEN || d->n_videos < 0) return VCT_E_SHAPE;
  if (!d->ids || !d->vid_rows || !d->vid_ref_ptr || !d->ref_tok_ptr || !d->ref_tok || !d->counts || !d->rouge) return VCT_E_ARG;
  if (!(d->beta_sq > 0.0)) return VCT_E_ARG;
  if (((uintptr_t)d->ids & 7) || ((uintptr_t)d->rouge & 7)) return VCT_E_ALIGN;
  if (((uintptr_t)d->vid_rows & 3) || ((uintptr_t)d->vid_ref_ptr & 3) || ((uintptr_t)d->ref_tok_ptr & 3) || ((uintptr_t)d->ref_tok & 3) ||
      ((uintptr_t)d->counts & 3))
    return VCT_E_ALIGN;
  vct::launch(capmetric_counts_kernel, dim3((unsigned)d->C), dim3(256), 0, (hipStream_t)stream, *d);
  VCT_CHECK_LAUNCH();
  return VCT_OK;
}

extern "C" int vct_capmetric_finish(int C, const int32_t* counts, const double* rouge, const double* cider, double* out, void* stream) {
  if (!counts || !rouge || !out) return VCT_E_ARG;
  if (C < 1) return VCT_E_SHAPE;
  if (((uintptr_t)rouge & 7) || ((uintptr_t)cider & 7) || ((uintptr_t)out & 7) || ((uintptr_t)counts & 3)) return VCT_E_ALIGN;
  vct::launch(capmetric_finish_kernel, dim3(1), dim3(CAPMETRIC_FINISH_THREADS), 0, (hipStream_t)stream, C, counts, rouge, cider, out);
  VCT_CHECK_LAUNCH();
  return VCT_OK;
}
