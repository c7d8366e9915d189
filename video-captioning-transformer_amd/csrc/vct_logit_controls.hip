// Generation controls for the KV-cached decode step on gfx950: repetition penalty, banned ids, minimum length and the
// no-repeat n-gram ban, applied in place to the step's logits between the generator and the selection kernels.
//
// replaces: nothing in the reference (it decodes greedily without any logit rule, MMT4Caption.py:146-184); the semantics are
// the project's (include/vct_hip.h, vct_logit_controls; decode.GenerationControls) and follow Hugging Face's logits processors
// of the same names.  Every setting is read from a 160-byte control block in device memory, so the captured per-position graphs
// serve every setting.
//
// A row has at most 64 history tokens: ONE WAVE PER ROW, lane l holds h[l].  The kernel touches at most 64 + 33 logits of a row
// and never sweeps V.
//   n-gram ban     lane j (n-1 <= j <= t-1) compares its n-1 predecessors with the suffix h[t-n+1 .. t-1]: n-1 shuffled compares,
//                  then one ballot of the matching lanes.
//   penalty        once per distinct token: lane l owns h[l] when no lower lane holds the same token (a lane-ordered compare over
//                  t broadcasts); the same pass tells the lane whether its token is n-gram banned.
//   ban set first  a lane penalises only a token that no rule bans, so no element is written twice with different values; lanes
//                  that ban the same token all store the same -inf.
// Rows (greedy / sampled sessions): 256-thread workgroups, four rows each, h[l] = ids[row][l].
// Beams: the history of a slot is its ancestors' tokens along the parent back-track.  An ancestor lies in the same video's K
// slots, so a workgroup per video stages that video's [t][K] parent and token columns in LDS (2 x 4 KB) and wave k walks slot
// k's chain there: t-1 dependent LDS reads instead of t-1 dependent L2 round trips per lane.
// No atomics, no workspace, plain vector stores.
#include "vct_common.h"

namespace vct {

constexpr int LC_HIST = 64;                 // history tokens per row: one per lane
constexpr int LC_KMAX = 16;                 // beams per video (vct_beam_select's limit)
constexpr int LC_NGRAM_MAX = 8;
constexpr int LC_BANNED_MAX = 32;
constexpr int LC_ROWS_PER_WG = 4;

// One row: `h` is this lane's history token (-1: no token, lane >= t or an id outside [0, V)).  All 64 lanes of the wave call.
template <typename T>
__device__ __forceinline__ void lc_apply_row(T* __restrict__ r, int h, int lane, int t, int V, int64_t end_id,
                                             const vct_logit_ctl* __restrict__ ctl) {
  const int min_length = ctl->min_length;
  int n = ctl->ngram;
  n = n < 0 ? 0 : (n > LC_NGRAM_MAX ? LC_NGRAM_MAX : n);
  int nb = ctl->n_banned;
  nb = nb < 0 ? 0 : (nb > LC_BANNED_MAX ? LC_BANNED_MAX : nb);
  const float theta = ctl->theta, inv_theta = ctl->inv_theta;
  const bool in_hist = lane < t;
  // ---- the ban set -------------------------------------------------------------------------------------------------------
  int bl = -1;                                                   // lane i < nb: banned id i
  if (lane < nb) {
    const int b = ctl->banned[lane];
    bl = (b >= 0 && b < V) ? b : -1;
  }
  const bool ban_end = t <= min_length && end_id >= 0 && end_id < (int64_t)V;
  bool match = false;                                            // lane j: h[j] would complete an n-gram the history holds
  if (n >= 1 && t >= n - 1) {
    match = in_hist && lane >= n - 1;
    for (int i = 1; i < n; i++) {                                // (uniform trip count: every lane shuffles)
      const int mine = __shfl(h, (lane - i) & 63);
      const int suffix = __shfl(h, (t - i) & 63);
      match = match && mine == suffix;
    }
  }
  const unsigned long long ng = __ballot(match);
  // ---- once per distinct token, and is that token banned ------------------------------------------------------------------
  bool first = in_hist && h >= 0;
  bool banned = ban_end && (int64_t)h == end_id;
  for (int j = 0; j < t; j++) {
    const int hj = __shfl(h, j);
    if (hj == h) {
      if (j < lane) first = false;
      if ((ng >> j) & 1ull) banned = true;
    }
  }
  for (int i = 0; i < nb; i++)
    if (__shfl(bl, i) == h) banned = true;
  // ---- stores --------------------------------------------------------------------------------------------------------------
  const T ninf = from_f<T>(-INFINITY);
  if (first && !banned && theta != 1.0f) {
    float x = to_f<T>(r[h]);
    x = x > 0.0f ? x * inv_theta : x * theta;
    r[h] = from_f<T>(x);
  }
  if (match && h >= 0) r[h] = ninf;
  if (bl >= 0) r[bl] = ninf;
  if (ban_end && lane == 0) r[end_id] = ninf;
}

__device__ __forceinline__ int lc_token(int64_t tok, int V) { return (tok >= 0 && tok < (int64_t)V) ? (int)tok : -1; }

template <typename T>
__global__ __launch_bounds__(LC_ROWS_PER_WG * 64) void logit_controls_rows_kernel(int rows, int V, T* __restrict__ x, int64_t ldx, int t,
                                                                                 int64_t end_id, const int64_t* __restrict__ ids,
                                                                                 int64_t ids_stride, const uint8_t* __restrict__ ended,
                                                                                 const vct_logit_ctl* __restrict__ ctl) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * LC_ROWS_PER_WG + (threadIdx.x >> 6);
  if (row >= rows || ended[row]) return;                          // (whole waves: no barrier below)
  const int h = lane < t ? lc_token(ids[(size_t)row * ids_stride + lane], V) : -1;
  lc_apply_row<T>(x + (size_t)row * ldx, h, lane, t, V, end_id, ctl);
}

template <typename T>
__global__ __launch_bounds__(LC_KMAX * 64) void logit_controls_beam_kernel(int K, int V, T* __restrict__ x, int64_t ldx, int t, int64_t end_id,
                                                                          const int64_t* __restrict__ ids, int64_t ids_stride,
                                                                          const uint8_t* __restrict__ finished,
                                                                          const int32_t* __restrict__ parents, int64_t parents_stride,
                                                                          const vct_logit_ctl* __restrict__ ctl) {
  __shared__ int s_tok[LC_HIST * LC_KMAX];      // [s][k]: the token slot k appended at step s (s = 0: the start token)
  __shared__ int s_par[LC_HIST * LC_KMAX];      // [s][k]: the slot of this video that slot k of step s continued
  const int lane = threadIdx.x & 63, k = threadIdx.x >> 6;
  const int row0 = blockIdx.x * K;
  for (int i = threadIdx.x; i < t * K; i += blockDim.x) {          // t <= 64, K <= 16: every index below stays inside the arrays
    const int s = i / K, kk = i - s * K;
    s_tok[s * LC_KMAX + kk] = lc_token(ids[(size_t)(row0 + kk) * ids_stride + s], V);
    int p = 0;
    if (s >= 1) {
      p = parents[(size_t)s * parents_stride + row0 + kk] - row0;
      p = p < 0 ? 0 : (p >= K ? K - 1 : p);                         // (a stale table cannot index outside the video)
    }
    s_par[s * LC_KMAX + kk] = p;
  }
  __syncthreads();
  const int row = row0 + k;
  if (finished[row]) return;
  // the back-track of decode.beam_decode_ids as of step t: h[s] = tok[s][r], r = par[s][r], for s = t-1 .. 1; h[0] = the start
  int r = k, h = -1;
  for (int s = t - 1; s >= 1; s--) {
    const int tok = s_tok[s * LC_KMAX + r];
    if (s == lane) h = tok;
    r = s_par[s * LC_KMAX + r];
  }
  if (lane == 0) h = s_tok[r];
  lc_apply_row<T>(x + (size_t)row * ldx, h, lane, t, V, end_id, ctl);
}

}  // namespace vct
using namespace vct;

extern "C" int vct_logit_controls(const vct_logit_controls_desc* d, void* stream) {
  if (!d || (d->dtype != VCT_F32 && d->dtype != VCT_BF16) || !d->x || !d->ids || !d->ended || !d->ctl) return VCT_E_ARG;
  const int rows = d->rows, V = d->V, t = d->t;
  if (rows <= 0 || V <= 0 || d->ldx < V || t < 1 || t > LC_HIST) return VCT_E_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  if (d->parents) {
    const int K = d->K;
    if (K < 1 || K > LC_KMAX || rows % K != 0) return VCT_E_SHAPE;
    const dim3 grid(rows / K), block(K * 64);
    if (d->dtype == VCT_BF16)
      vct::launch((logit_controls_beam_kernel<bf16_t>), grid, block, 0, st, K, V, (bf16_t*)d->x, d->ldx, t, d->end_id, d->ids, d->ids_stride,
                  d->ended, d->parents, d->parents_stride, d->ctl);
    else
      vct::launch((logit_controls_beam_kernel<float>), grid, block, 0, st, K, V, (float*)d->x, d->ldx, t, d->end_id, d->ids, d->ids_stride,
                  d->ended, d->parents, d->parents_stride, d->ctl);
  } else {
    const dim3 grid((rows + LC_ROWS_PER_WG - 1) / LC_ROWS_PER_WG), block(LC_ROWS_PER_WG * 64);
    if (d->dtype == VCT_BF16)
      vct::launch((logit_controls_rows_kernel<bf16_t>), grid, block, 0, st, rows, V, (bf16_t*)d->x, d->ldx, t, d->end_id, d->ids,
                  d->ids_stride, d->ended, d->ctl);
    else
      vct::launch((logit_controls_rows_kernel<float>), grid, block, 0, st, rows, V, (float*)d->x, d->ldx, t, d->end_id, d->ids,
                  d->ids_stride, d->ended, d->ctl);
  }
  VCT_CHECK_LAUNCH();
  return VCT_OK;
}
