// Head-averaged attention probabilities W[b, i, j] = (1/H) sum_h softmax_j(q[b,i,h] . k[b,j,h] / sqrt(hd) + mask) on gfx950:
// what nn.MultiheadAttention hands back with need_weights=True, average_attn_weights=True.  The mean over heads is a reduction
// ACROSS the (batch, head) workgroups of vct_attn_fwd, so it is a kernel of its own: one wave per (batch, 16-query tile) walks
// the heads in ascending order, stages that head's Q tile and K slice into LDS (16-byte loads, vct_attn_core.h), rebuilds the
// S^T tiles, masks, row maximum, exponentials and 1 / row sum with the very helpers the forward uses, and adds P into fp32
// registers.  No atomics and no second pass: the summation order is fixed, two runs are bitwise equal, and a map is exactly the
// probability the forward multiplied V with at p_drop = 0.  A fully masked row gives zeros (inv = 0), never NaN.
//
// S^T layout (scores_T): a lane holds ONE query (qt*16 + (lane & 15)) and, per key tile t, the four keys t*16 + (lane >> 4)*4 + r
// -- four consecutive fp32 of an output row.  The Q region of LDS is addressed by the query's row in the whole sequence (scores_T
// and the causal mask index it that way); only this workgroup's tile of it is staged and read.
#include "vct_attn_core.h"

namespace vct {

struct AttnWOut { float* w; long ldw, w_bs; };

template <typename T, int DT> static size_t attn_weights_lds_bytes(int Lq, int Lk) {
  using C = AttnCfg<T, DT>;
  return (size_t)(((Lq + 15) / 16) * 16 + ((Lk + 15) / 16) * 16) * C::STR * sizeof(T);
}

template <typename T, int DT>
__global__ __launch_bounds__(64) void attn_weights_kernel(const AttnP p, const AttnWOut o) {
  using C = AttnCfg<T, DT>;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = threadIdx.x, i = lane & 15, g = lane >> 4;
  const int LQT = (p.Lq + 15) / 16, LKT = (p.Lk + 15) / 16;
  const int b = blockIdx.x / LQT, qt = blockIdx.x % LQT;
  T* Qs = reinterpret_cast<T*>(smem);
  T* Ks = Qs + LQT * 16 * C::STR;
  const T* qg = reinterpret_cast<const T*>(p.q) + (long)b * p.q_bs + (long)qt * 16 * p.ldq;
  const T* kg = reinterpret_cast<const T*>(p.k) + (long)b * p.k_bs;
  const int q_rows = min(16, p.Lq - qt * 16);
  const unsigned long long kp_row = load_padmask(p, b, lane);
  const float scale = 1.0f / sqrtf((float)p.hd);
  const int hd4 = (p.hd + 3) / 4;

  f32x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; t++) acc[t] = f32x4{0, 0, 0, 0};

  for (int h = 0; h < p.H; h++) {
    if (h > 0) __syncthreads();            // the previous head's fragments have been read
    {
      const StageJob<T> jobs[2] = {{Qs + qt * 16 * C::STR, qg + (long)h * p.hd, p.ldq, q_rows, 16},
                                   {Ks, kg + (long)h * p.hd, p.ldk, p.Lk, LKT * 16}};
      stage_multi<T, DT, 2>(jobs, p.hd, lane);
    }
    __syncthreads();
    f32x4 st[4];
    scores_T<T, DT>(st, Ks, Qs, qt, LKT, hd4, scale, p, kp_row, lane);
    float m = -INFINITY;
#pragma unroll
    for (int t = 0; t < 4; t++)
#pragma unroll
      for (int r = 0; r < 4; r++) m = fmaxf(m, st[t][r]);
    m = red4_max(m);
    if (m == -INFINITY) m = 0.0f;
    float l = 0.0f;
#pragma unroll
    for (int t = 0; t < 4; t++) {
      if (t < LKT) {
#pragma unroll
        for (int r = 0; r < 4; r++) { st[t][r] = attn_exp<T>(st[t][r] - m); l += st[t][r]; }
      } else {
        st[t] = f32x4{0, 0, 0, 0};
      }
    }
    l = red4_sum(l);
    const float inv = l > 0.0f ? 1.0f / l : 0.0f;
#pragma unroll
    for (int t = 0; t < 4; t++)
#pragma unroll
      for (int r = 0; r < 4; r++) acc[t][r] += st[t][r] * inv;
  }

  const int qq = qt * 16 + i;
  const float inv_h = 1.0f / (float)p.H;
  if (qq < p.Lq) {
    float* wrow = o.w + (long)b * o.w_bs + (long)qq * o.ldw;
#pragma unroll
    for (int t = 0; t < 4; t++)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int kk = t * 16 + g * 4 + r;
        if (kk < p.Lk) wrow[kk] = acc[t][r] * inv_h;
      }
  }
}

template <typename T, int DT> static int attn_weights_launch(const AttnP& p, const AttnWOut& o, hipStream_t st) {
  const size_t lds = attn_weights_lds_bytes<T, DT>(p.Lq, p.Lk);
  if (lds > 160 * 1024) return VCT_E_SHAPE;
  if (lds > 64 * 1024) {       // fp32 at the shape limits only: opt in once per device (the attribute is a maximum, not a request)
    static vct::DynLdsOptIn optin;
    if (hipError_t e = optin.ensure((const void*)attn_weights_kernel<T, DT>, 160 * 1024); e != hipSuccess) return (int)e;
  }
  const int LQT = (p.Lq + 15) / 16;
  vct::launch((attn_weights_kernel<T, DT>), dim3(p.B * LQT), dim3(64), lds, st, p, o);
  VCT_CHECK_LAUNCH();
  return VCT_OK;
}

template <typename T> static int attn_weights_dispatch(const AttnP& p, const AttnWOut& o, hipStream_t st) {
  if (p.hd <= 16) return attn_weights_launch<T, 1>(p, o, st);
  if (p.hd <= 32) return attn_weights_launch<T, 2>(p, o, st);
  if (p.hd <= 64) return attn_weights_launch<T, 4>(p, o, st);
  if (p.hd <= 96) return attn_weights_launch<T, 6>(p, o, st);
  if (p.hd <= 128) return attn_weights_launch<T, 8>(p, o, st);
  return VCT_E_SHAPE;
}

}  // namespace vct
using namespace vct;

extern "C" int vct_attn_weights(const vct_attn_weights_desc* d, void* stream) {
  if (!d || !d->q || !d->k || !d->w) return VCT_E_ARG;
  if (d->dtype != VCT_F32 && d->dtype != VCT_BF16) return VCT_E_ARG;
  if (d->B <= 0 || d->H <= 0 || d->Lq <= 0 || d->Lk <= 0 || d->hd <= 0) return VCT_E_SHAPE;
  if (d->Lq > 64 || d->Lk > 64 || d->hd > 128) return VCT_E_SHAPE;
  if (d->ldw < d->Lk) return VCT_E_SHAPE;
  const int vec = d->dtype == VCT_BF16 ? 8 : 4;
  if (d->hd % vec || d->ldq % vec || d->ldk % vec || d->q_bs % vec || d->k_bs % vec) return VCT_E_ALIGN;
  if (((uintptr_t)d->q | (uintptr_t)d->k) & 15) return VCT_E_ALIGN;
  if ((uintptr_t)d->w & 3) return VCT_E_ALIGN;
  if (d->key_pad_shift < 0 || (d->key_pad != nullptr && d->key_pad_shift >= d->Lk)) return VCT_E_SHAPE;
  AttnP p = {};
  p.B = d->B; p.H = d->H; p.Lq = d->Lq; p.Lk = d->Lk; p.hd = d->hd; p.causal = d->causal;
  p.q = d->q; p.ldq = d->ldq; p.k = d->k; p.ldk = d->ldk;
  p.key_pad = d->key_pad; p.key_pad_shift = d->key_pad_shift;
  p.key_ids = d->key_ids; p.key_ids_bs = d->key_ids_bs; p.pad_id = d->pad_id;
  p.q_bs = d->q_bs ? d->q_bs : (long)d->Lq * d->ldq;
  p.k_bs = d->k_bs ? d->k_bs : (long)d->Lk * d->ldk;
  AttnWOut o;
  o.w = d->w; o.ldw = d->ldw;
  o.w_bs = d->w_bs ? d->w_bs : (long)d->Lq * d->ldw;
  hipStream_t st = (hipStream_t)stream;
  return d->dtype == VCT_BF16 ? attn_weights_dispatch<bf16_t>(p, o, st) : attn_weights_dispatch<float>(p, o, st);
}
