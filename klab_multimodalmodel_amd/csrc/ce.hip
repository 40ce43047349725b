// LM-head cross-entropy (HF/t5:1050-1054: CrossEntropyLoss(ignore_index=-100), mean over the non-ignored rows; pads (id 0) ARE
// scored), with d logits written in place: one kernel family behind klab_ce_count, klab_ce_fwd, klab_ce_wsum,
// klab_ce_fwd_opts and klab_ce_fwd_distill.
//
// plain (klab_ce_fwd): the options below at eps = 0, z = 0, no weights
//   l_i     = lse - x_y                                                     (0 where y == -100)
//   loss    = sum_i l_i / n,   n = number of labels != -100                 (0 when n == 0)
//   dl/dx_j = (p_j - delta_jy) / n
//
// options (klab_ce_fwd_opts): label smoothing eps, z-loss z and per-row weights w (NULL = all ones)
//   l_i     = lse - (1 - eps) x_y - (eps / V) sum_j x_j + z lse^2           (0 where y == -100)
//   loss    = sum_i w_i l_i / W,   W = sum_{i : y_i != -100} w_i            (0 when W == 0)
//   dl/dx_j = (w_i / W) [ p_j (1 + 2 z lse) - (1 - eps) delta_jy - eps / V ]
//
// distillation (klab_ce_fwd_distill): the options' l as ce, mixed with the KL divergence from a teacher's logits t [rows, V]
// (read-only, bf16 or f32, its own row stride) at temperature T, in the same pass over the student's row
//   p       = softmax(t / T),  q = softmax(x / T)
//   kl      = sum_j p_j (log p_j - log q_j) = (1 / T) (sum_j p_j (t_j - x_j) - (max t - max x)) - log st + log sq
//             with st = sum_j exp((t_j - max t) / T), sq = sum_j exp((x_j - max x) / T)
//   l       = (1 - alpha) ce + alpha T^2 kl                                 (0 where y == -100)
//   dl/dx_j = (w_i / W) [ (1 - alpha) (the options' bracket) + alpha T (q_j - p_j) ]
//
// Two forms: register-resident one-pass for bf16 rows up to 32768 logits (V <= 256 lanes * 16 bytes * NIT; the T5 vocabulary is
// 32128): the row -- and the teacher's beside it -- is read ONCE, every load issued before the first use, and d logits are written
// from the registers; two-pass (online soft-max) above that and for f32, which re-reads the row (4096 rows x 64 KB in flight do not
// fit the L2s: 790 MB of traffic for 526 MB of algorithmic bytes).  Both exist without a teacher (ce_kernel, ce_onepass_kernel; SX: the
// row sum of the logits is wanted, eps != 0) and with one (ce_kd_kernel, ce_kd_onepass_kernel: the same operations on x in the
// same order with the teacher's row beside the student's), built from one set of device functions.  Exponentials per logit: 2 without a teacher; with one 4 at T == 1 (exp(x - max),
// exp(t - max) for the sums; exp(x - lse), exp(t - lse_t) for the gradient -- q is softmax(x) there and sq the cross-entropy's sum),
// 6 otherwise (exp((x - max) / T) and q_j on top).
//
// klab_ce_fwd IS klab_ce_fwd_opts at neutral options, which give the plain loss: every added operation is exact -- 1 - eps = 1, eps / V = 0, z lse = 0, 1 + 2 z lse = 1 and w inv_w = inv_n -- so each
// expression rounds once where lse - x_y, p_j g and (p_y - 1) g round once.  alpha == 0 is the options' loss: the cross-entropy
// part joins as (1 - alpha) a + alpha b, where 1 - alpha = 1 and alpha b = 0 (the teacher is finite); a row with g = w / W == 0
// takes the cross-entropy's value alone, so that the sign of its zeros is the same too.  With a teacher equal to the student's
// logits the large terms vanish instead of cancelling: t_j - x_j = 0 and the maxima agree, which leaves log sq - log st, two sums
// of the same values.
#include <math.h>
#include <stdint.h>

#include <type_traits>

#include "common.h"
#include "klab_mm.h"

namespace klab {
namespace {

struct CeOpts {
  float ome;   // 1 - eps
  float epsv;  // eps / V
  float z;
};
struct KdOpts {
  float alpha, oma;  // oma = 1 - alpha
  float T, invT;
  float aT2;  // alpha T^2
};

// inv_w[0] = 1 / sum of the weights of the rows with a label, 0 when that sum is 0.  One workgroup, fixed order.  Weights of all
// ones (or NULL: klab_ce_count, klab_ce_fwd) sum to the exact count (< 2^24), so the quotient is 1 / (float)n of the integer count.
__global__ __launch_bounds__(256) void ce_norm_kernel(const long long* __restrict__ labels, const float* __restrict__ weights, int rows,
                                                      float* __restrict__ inv_w) {
  __shared__ float red[4];
  float a = 0.f;
  for (int i = threadIdx.x; i < rows; i += 256) a += labels[i] != -100 ? (weights ? weights[i] : 1.f) : 0.f;
  a = wave_sum(a);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float W = red[0] + red[1] + red[2] + red[3];
    inv_w[0] = W > 0.f ? 1.f / W : 0.f;   // (the reference would produce NaN for W == 0)
  }
}

// loss[0] = (sum_i w_i l_i) inv_w (rows without a label hold l = 0)
__global__ __launch_bounds__(256) void ce_reduce_kernel(const float* __restrict__ loss_row, const float* __restrict__ weights, int rows,
                                                        const float* __restrict__ inv_w, float* __restrict__ loss) {
  __shared__ float red[4];
  float a = 0.f;
  for (int i = threadIdx.x; i < rows; i += 256) a += weights ? weights[i] * loss_row[i] : loss_row[i];  // fixed order => bit-reproducible
  a = wave_sum(a);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) loss[0] = (red[0] + red[1] + red[2] + red[3]) * inv_w[0];
}

// ---- the cross-entropy part ----------------------------------------------------------------------------------------------------
// Which of these multiply-adds are fused is spelled out, like the gradient's below: left to the compiler's contraction it depends
// on what the vectoriser pairs them with, instantiation by instantiation.  The two products round on their own, the z term is fused.
__device__ __forceinline__ float row_loss(float lse, float xlab, float sx, const CeOpts& o) {
#pragma clang fp contract(off)
  float l = lse - o.ome * xlab;
  l -= o.epsv * sx;
  return __builtin_fmaf(o.z * lse, lse, l);
}

// The gradient of a row is g [p_j k - (1 - eps) delta_jy - eps / V] with g = w inv_w and k = 1 + 2 z lse.  Off the label that is
// ONE fused multiply-add per element, p_j (g k) - g eps / V -- p_j g when the options are neutral, and exact zeros when g == 0 --
// and the label's element is mended afterwards by the one lane that holds it, as ((p_y k - (1 - eps)) - eps / V) g: (p_y - 1) g
// with neutral options, two roundings.  The kernels are VALU-bound next to their __expf per logit, so the label is looked for
// once per 16-byte vector, not once per element.
struct GradCoef {
  float gk, ge, k, g;
};
__device__ __forceinline__ GradCoef grad_coef(float lse, float g, const CeOpts& o) {
  const float k = 1.f + 2.f * (o.z * lse);
  return GradCoef{g * k, g * o.epsv, k, g};
}
// The two multiply-adds are spelled out: left to the compiler's contraction, the same source expression was fused in every
// instantiation without a teacher but in only half of the f32 kernel's elements beside the distillation term, one unit in the last
// place apart.
__device__ __forceinline__ float ce_elem(float pr, const GradCoef& q) { return __builtin_fmaf(pr, q.gk, -q.ge); }
__device__ __forceinline__ float grad_at_label(float pr, const GradCoef& q, const CeOpts& o) {
  float t = __builtin_fmaf(pr, q.k, -o.ome);
  t -= o.epsv;
  return t * q.g;
}

// ---- without a teacher.  SX: the row sum of the logits is wanted (eps != 0) ----------------------------------------------------
// two-pass form: online soft-max of the row, then the gradient
template <typename T, bool SX>
__global__ __launch_bounds__(256) void ce_kernel(T* __restrict__ logits, long ld, const long long* __restrict__ labels,
                                                      const float* __restrict__ weights, int V, CeOpts o, const float* __restrict__ inv_w,
                                                      float* __restrict__ loss_row, int write_grad) {
  constexpr int VEC = Vec16<T>::N;
  using VT = typename Vec16<T>::type;
  __shared__ float red[12];
  const long row = blockIdx.x;
  const int tid = threadIdx.x;
  T* x = logits + row * ld;
  const long long lab = labels[row];
  const bool valid = lab != -100;
  // (issued ahead of the row: nothing waits for them behind the reduction)
  const float g = write_grad && valid ? (weights ? weights[row] : 1.f) * inv_w[0] : 0.f;
  float m = -INFINITY, s = 0.f, sx = 0.f;
  for (int c = tid * VEC; c < V; c += 256 * VEC) {
    VT v = *reinterpret_cast<const VT*>(x + c);
    float mx = to_f32(v[0]);
#pragma unroll
    for (int u = 1; u < VEC; ++u) mx = fmaxf(mx, to_f32(v[u]));
    const float mn = fmaxf(m, mx);
    float a = 0.f;
#pragma unroll
    for (int u = 0; u < VEC; ++u) {
      a += __expf(to_f32(v[u]) - mn);
      if constexpr (SX) sx += to_f32(v[u]);
    }
    s = s * __expf(m - mn) + a;
    m = mn;
  }
  float wm = wave_max(m);
  float ws = wave_sum(m == -INFINITY ? 0.f : s * __expf(m - wm));  // lanes/waves with no column contribute 0, not NaN
  const float wx = SX ? wave_sum(sx) : 0.f;
  if ((tid & 63) == 0) { red[tid >> 6] = wm; red[4 + (tid >> 6)] = ws; red[8 + (tid >> 6)] = wx; }
  __syncthreads();
  const float bm = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  float bs = 0.f;
#pragma unroll
  for (int w = 0; w < 4; ++w) bs += red[w] == -INFINITY ? 0.f : red[4 + w] * __expf(red[w] - bm);
  const float lse = bm + __logf(bs);
  const float bsx = red[8] + red[9] + red[10] + red[11];
  if (tid == 0) loss_row[row] = valid ? row_loss(lse, to_f32(x[lab]), bsx, o) : 0.f;
  if (!write_grad) return;
  __syncthreads();  // x[lab] read above before it is overwritten below
  const GradCoef q = grad_coef(lse, g, o);
  const int labi = (int)lab;
  for (int c = tid * VEC; c < V; c += 256 * VEC) {
    VT v = *reinterpret_cast<const VT*>(x + c);
    VT out;
#pragma unroll
    for (int u = 0; u < VEC; ++u) out[u] = from_f32<T>(ce_elem(__expf(to_f32(v[u]) - lse), q));
    const unsigned at = (unsigned)(labi - c);
    if (at < (unsigned)VEC) {
#pragma unroll
      for (int u = 0; u < VEC; ++u)
        if (u == (int)at) out[u] = from_f32<T>(grad_at_label(__expf(to_f32(v[u]) - lse), q, o));
    }
    *reinterpret_cast<VT*>(x + c) = out;
  }
}

// one-pass form: every load of the row is issued before the first use, d logits leave the registers
template <typename T, int NIT, bool SX>
__global__ __launch_bounds__(256) void ce_onepass_kernel(T* __restrict__ logits, long ld, const long long* __restrict__ labels,
                                                              const float* __restrict__ weights, int V, CeOpts o,
                                                              const float* __restrict__ inv_w, float* __restrict__ loss_row, int write_grad) {
  constexpr int VEC = Vec16<T>::N;
  using VT = typename Vec16<T>::type;
  __shared__ float red[12];
  __shared__ float xlab;
  const long row = blockIdx.x;
  const int tid = threadIdx.x;
  T* x = logits + row * ld;
  const long long lab = labels[row];
  const int labi = (int)lab;
  const bool valid = lab != -100;
  VT v[NIT];
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int c = (it * 256 + tid) * VEC;
    if (c < V) v[it] = *reinterpret_cast<const VT*>(x + c);
  }
  const float g = write_grad && valid ? (weights ? weights[row] : 1.f) * inv_w[0] : 0.f;  // (in flight with the row)
  float m = -INFINITY;
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int c = (it * 256 + tid) * VEC;
    if (c < V) {
#pragma unroll
      for (int u = 0; u < VEC; ++u) m = fmaxf(m, to_f32(v[it][u]));
    }
  }
  const float wm = wave_max(m);
  if ((tid & 63) == 0) red[tid >> 6] = wm;
  __syncthreads();
  const float bm = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  float sum = 0.f, sx = 0.f;
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int c = (it * 256 + tid) * VEC;
    if (c < V) {
#pragma unroll
      for (int u = 0; u < VEC; ++u) {
        const float xv = to_f32(v[it][u]);
        sum += __expf(xv - bm);
        if constexpr (SX) sx += xv;
      }
      const unsigned at = (unsigned)(labi - c);
      if (at < (unsigned)VEC) {
#pragma unroll
        for (int u = 0; u < VEC; ++u)
          if (u == (int)at) xlab = to_f32(v[it][u]);
      }
    }
  }
  const float ws = wave_sum(sum);
  const float wx = SX ? wave_sum(sx) : 0.f;
  if ((tid & 63) == 0) { red[4 + (tid >> 6)] = ws; red[8 + (tid >> 6)] = wx; }
  __syncthreads();
  const float lse = bm + __logf(red[4] + red[5] + red[6] + red[7]);
  const float bsx = red[8] + red[9] + red[10] + red[11];
  if (tid == 0) loss_row[row] = valid ? row_loss(lse, xlab, bsx, o) : 0.f;
  if (!write_grad) return;
  const GradCoef q = grad_coef(lse, g, o);
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int c = (it * 256 + tid) * VEC;
    if (c < V) {
      VT out;
#pragma unroll
      for (int u = 0; u < VEC; ++u) out[u] = from_f32<T>(ce_elem(__expf(to_f32(v[it][u]) - lse), q));
      const unsigned at = (unsigned)(labi - c);
      if (at < (unsigned)VEC) {
#pragma unroll
        for (int u = 0; u < VEC; ++u)
          if (u == (int)at) out[u] = from_f32<T>(grad_at_label(__expf(to_f32(v[it][u]) - lse), q, o));
      }
      *reinterpret_cast<VT*>(x + c) = out;
    }
  }
}

// ---- the teacher's values beside one 16-byte vector of the student (N = 8 bf16 or 4 f32 logits) --------------------------------
template <typename TT, int N> struct TVec;
template <> struct TVec<bf16_t, 8> {
  bf16x8 v;
  __device__ __forceinline__ void load(const bf16_t* p) { v = *reinterpret_cast<const bf16x8*>(p); }
  __device__ __forceinline__ float get(int u) const { return (float)v[u]; }
};
template <> struct TVec<float, 8> {
  f32x4 a, b;
  __device__ __forceinline__ void load(const float* p) { a = *reinterpret_cast<const f32x4*>(p); b = *reinterpret_cast<const f32x4*>(p + 4); }
  __device__ __forceinline__ float get(int u) const { return u < 4 ? a[u & 3] : b[u & 3]; }
};
template <> struct TVec<bf16_t, 4> {
  bf16x4 v;
  __device__ __forceinline__ void load(const bf16_t* p) { v = *reinterpret_cast<const bf16x4*>(p); }
  __device__ __forceinline__ float get(int u) const { return (float)v[u]; }
};
template <> struct TVec<float, 4> {
  f32x4 v;
  __device__ __forceinline__ void load(const float* p) { v = *reinterpret_cast<const f32x4*>(p); }
  __device__ __forceinline__ float get(int u) const { return v[u]; }
};
// what a row knows after its sums
struct RowStat {
  float lse;   // of x (the cross-entropy's)
  float lqT;   // max x / T + log sq: q_j = exp(x_j / T - lqT)     (TEMP only)
  float ltT;   // max t / T + log st: p_j = exp(t_j / T - ltT)
  float kl;
};
// bm, sum: the cross-entropy's maximum and sum of exp(x - bm); sq: sum of exp((x - bm) / T) (TEMP; otherwise `sum`)
template <bool TEMP>
__device__ __forceinline__ RowStat row_stat(float bm, float sum, float sq, float tm, float st, float dot, const KdOpts& k) {
  RowStat r;
  const float lsum = __logf(sum);
  r.lse = bm + lsum;
  const float lst = __logf(st);
  const float lsq = TEMP ? __logf(sq) : lsum;
  const float s = dot / st;  // sum_j p_j (t_j - x_j)
  if constexpr (TEMP) {
    r.kl = __builtin_fmaf(s - (tm - bm), k.invT, -lst) + lsq;
    r.lqT = bm * k.invT + lsq;
    r.ltT = tm * k.invT + lst;
  } else {
    r.kl = ((s - (tm - bm)) - lst) + lsq;
    r.lqT = r.lse;
    r.ltT = tm + lst;
  }
  return r;
}

// one element of the gradient.  a: the cross-entropy's element, e = exp(x - lse)
template <bool TEMP>
__device__ __forceinline__ float kd_join(float a, float e, float xv, float tv, const RowStat& r, const KdOpts& k, float c2, bool live) {
  float out = k.oma * a;
  if (live) {
    const float q = TEMP ? __expf(xv * k.invT - r.lqT) : e;
    const float p = TEMP ? __expf(tv * k.invT - r.ltT) : __expf(tv - r.ltT);
    out += c2 * (q - p);  // c2 = alpha (g T)
  }
  return out;
}

// l = (1 - alpha) ce + alpha T^2 kl: two products and their sum, each rounded (spelled out like row_loss)
__device__ __forceinline__ float kd_row_loss(float ce, float kl, const KdOpts& k) {
#pragma clang fp contract(off)
  return k.oma * ce + k.aT2 * kl;
}

// ---- with a teacher: the kernels above with the teacher's row beside the student's --------------------------------------------
// two-pass form: online soft-max of both rows, then the gradient
template <typename T, typename TT, bool SX, bool TEMP>
__global__ __launch_bounds__(256) void ce_kd_kernel(T* __restrict__ logits, long ld, const TT* __restrict__ teacher, long ldt,
                                                         const long long* __restrict__ labels, const float* __restrict__ weights, int V,
                                                         CeOpts o, KdOpts kd, const float* __restrict__ inv_w, float* __restrict__ loss_row,
                                                         float* __restrict__ kl_row, int write_grad) {
  constexpr int VEC = Vec16<T>::N;
  using VT = typename Vec16<T>::type;
  __shared__ float red[28];
  const long row = blockIdx.x;
  const int tid = threadIdx.x;
  T* x = logits + row * ld;
  const TT* t = teacher + row * ldt;
  const long long lab = labels[row];
  const bool valid = lab != -100;
  const float g = write_grad && valid ? (weights ? weights[row] : 1.f) * inv_w[0] : 0.f;
  float m = -INFINITY, s = 0.f, sx = 0.f;        // the cross-entropy's (ce_kernel)
  float sq = 0.f;                                // sum exp((x - m) / T)
  float mt = -INFINITY, st = 0.f, dot = 0.f;     // the teacher's maximum, sum exp((t - mt) / T) and sum exp(..) (t - x)
  for (int c = tid * VEC; c < V; c += 256 * VEC) {
    VT v = *reinterpret_cast<const VT*>(x + c);
    TVec<TT, VEC> tv;
    tv.load(t + c);
    float mx = to_f32(v[0]), mxt = tv.get(0);
#pragma unroll
    for (int u = 1; u < VEC; ++u) { mx = fmaxf(mx, to_f32(v[u])); mxt = fmaxf(mxt, tv.get(u)); }
    const float mn = fmaxf(m, mx), mtn = fmaxf(mt, mxt);
    float a = 0.f, aq = 0.f, at = 0.f, ad = 0.f;
#pragma unroll
    for (int u = 0; u < VEC; ++u) {
      const float xv = to_f32(v[u]), tu = tv.get(u);
      a += __expf(xv - mn);
      if constexpr (SX) sx += xv;
      if constexpr (TEMP) aq += __expf((xv - mn) * kd.invT);
      const float et = TEMP ? __expf((tu - mtn) * kd.invT) : __expf(tu - mtn);
      at += et;
      ad += et * (tu - xv);
    }
    s = s * __expf(m - mn) + a;
    if constexpr (TEMP) sq = sq * __expf((m - mn) * kd.invT) + aq;
    const float ft = TEMP ? __expf((mt - mtn) * kd.invT) : __expf(mt - mtn);
    st = st * ft + at;
    dot = dot * ft + ad;
    m = mn;
    mt = mtn;
  }
  const float wm = wave_max(m), wmt = wave_max(mt);
  const float ws = wave_sum(m == -INFINITY ? 0.f : s * __expf(m - wm));  // lanes/waves with no column contribute 0, not NaN
  const float wx = SX ? wave_sum(sx) : 0.f;
  const float wq = TEMP ? wave_sum(m == -INFINITY ? 0.f : sq * __expf((m - wm) * kd.invT)) : 0.f;
  const float fl = mt == -INFINITY ? 0.f : (TEMP ? __expf((mt - wmt) * kd.invT) : __expf(mt - wmt));
  const float wst = wave_sum(st * fl), wd = wave_sum(dot * fl);
  if ((tid & 63) == 0) {
    const int w = tid >> 6;
    red[w] = wm; red[4 + w] = ws; red[8 + w] = wx; red[12 + w] = wq; red[16 + w] = wmt; red[20 + w] = wst; red[24 + w] = wd;
  }
  __syncthreads();
  const float bm = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  const float tm = fmaxf(fmaxf(red[16], red[17]), fmaxf(red[18], red[19]));
  float bs = 0.f, bq = 0.f, bst = 0.f, bd = 0.f;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    bs += red[w] == -INFINITY ? 0.f : red[4 + w] * __expf(red[w] - bm);
    if constexpr (TEMP) bq += red[w] == -INFINITY ? 0.f : red[12 + w] * __expf((red[w] - bm) * kd.invT);
    const float f = red[16 + w] == -INFINITY ? 0.f : (TEMP ? __expf((red[16 + w] - tm) * kd.invT) : __expf(red[16 + w] - tm));
    bst += red[20 + w] * f;
    bd += red[24 + w] * f;
  }
  const RowStat r = row_stat<TEMP>(bm, bs, bq, tm, bst, bd, kd);
  const float lse = r.lse;
  const float bsx = red[8] + red[9] + red[10] + red[11];
  if (tid == 0) {
    const float ce = valid ? row_loss(lse, to_f32(x[lab]), bsx, o) : 0.f;
    loss_row[row] = valid ? kd_row_loss(ce, r.kl, kd) : 0.f;
    kl_row[row] = valid ? r.kl : 0.f;
  }
  if (!write_grad) return;
  __syncthreads();  // x[lab] read above before it is overwritten below
  const GradCoef q = grad_coef(lse, g, o);
  const bool live = g != 0.f;
  const float c2 = kd.alpha * (g * kd.T);
  const int labi = (int)lab;
  for (int c = tid * VEC; c < V; c += 256 * VEC) {
    VT v = *reinterpret_cast<const VT*>(x + c);
    TVec<TT, VEC> tv;
    tv.load(t + c);
    VT out;
#pragma unroll
    for (int u = 0; u < VEC; ++u) {
      const float xv = to_f32(v[u]), e = __expf(xv - lse);
      out[u] = from_f32<T>(kd_join<TEMP>(ce_elem(e, q), e, xv, tv.get(u), r, kd, c2, live));
    }
    const unsigned at = (unsigned)(labi - c);
    if (at < (unsigned)VEC) {
#pragma unroll
      for (int u = 0; u < VEC; ++u)
        if (u == (int)at) {
          const float xv = to_f32(v[u]), e = __expf(xv - lse);
          out[u] = from_f32<T>(kd_join<TEMP>(grad_at_label(e, q, o), e, xv, tv.get(u), r, kd, c2, live));
        }
    }
    *reinterpret_cast<VT*>(x + c) = out;
  }
}

// one-pass form: every load of both rows is issued before the first use, d logits leave the registers
template <typename TT, int NIT, bool SX, bool TEMP>
__global__ __launch_bounds__(256) void ce_kd_onepass_kernel(bf16_t* __restrict__ logits, long ld, const TT* __restrict__ teacher, long ldt,
                                                                 const long long* __restrict__ labels, const float* __restrict__ weights,
                                                                 int V, CeOpts o, KdOpts kd, const float* __restrict__ inv_w,
                                                                 float* __restrict__ loss_row, float* __restrict__ kl_row, int write_grad) {
  using T = bf16_t;
  constexpr int VEC = 8;
  using VT = bf16x8;
  __shared__ float red[28];
  __shared__ float xlab;
  const long row = blockIdx.x;
  const int tid = threadIdx.x;
  T* x = logits + row * ld;
  const TT* t = teacher + row * ldt;
  const long long lab = labels[row];
  const int labi = (int)lab;
  const bool valid = lab != -100;
  VT v[NIT];
  TVec<TT, VEC> tv[NIT];
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int c = (it * 256 + tid) * VEC;
    if (c < V) { v[it] = *reinterpret_cast<const VT*>(x + c); tv[it].load(t + c); }
  }
  const float g = write_grad && valid ? (weights ? weights[row] : 1.f) * inv_w[0] : 0.f;  // (in flight with the rows)
  float m = -INFINITY, mt = -INFINITY;
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int c = (it * 256 + tid) * VEC;
    if (c < V) {
#pragma unroll
      for (int u = 0; u < VEC; ++u) { m = fmaxf(m, to_f32(v[it][u])); mt = fmaxf(mt, tv[it].get(u)); }
    }
  }
  const float wm = wave_max(m), wmt = wave_max(mt);
  if ((tid & 63) == 0) { red[tid >> 6] = wm; red[16 + (tid >> 6)] = wmt; }
  __syncthreads();
  const float bm = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  const float tm = fmaxf(fmaxf(red[16], red[17]), fmaxf(red[18], red[19]));
  float sum = 0.f, sx = 0.f, sq = 0.f, st = 0.f, dot = 0.f;
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int c = (it * 256 + tid) * VEC;
    if (c < V) {
#pragma unroll
      for (int u = 0; u < VEC; ++u) {
        const float xv = to_f32(v[it][u]), tu = tv[it].get(u);
        sum += __expf(xv - bm);
        if constexpr (SX) sx += xv;
        if constexpr (TEMP) sq += __expf((xv - bm) * kd.invT);
        const float et = TEMP ? __expf((tu - tm) * kd.invT) : __expf(tu - tm);
        st += et;
        dot += et * (tu - xv);
      }
      const unsigned at = (unsigned)(labi - c);
      if (at < (unsigned)VEC) {
#pragma unroll
        for (int u = 0; u < VEC; ++u)
          if (u == (int)at) xlab = to_f32(v[it][u]);
      }
    }
  }
  const float ws = wave_sum(sum);
  const float wx = SX ? wave_sum(sx) : 0.f;
  const float wq = TEMP ? wave_sum(sq) : 0.f;
  const float wst = wave_sum(st), wd = wave_sum(dot);
  if ((tid & 63) == 0) {
    const int w = tid >> 6;
    red[4 + w] = ws; red[8 + w] = wx; red[12 + w] = wq; red[20 + w] = wst; red[24 + w] = wd;
  }
  __syncthreads();
  const RowStat r = row_stat<TEMP>(bm, red[4] + red[5] + red[6] + red[7], red[12] + red[13] + red[14] + red[15], tm,
                                   red[20] + red[21] + red[22] + red[23], red[24] + red[25] + red[26] + red[27], kd);
  const float lse = r.lse;
  const float bsx = red[8] + red[9] + red[10] + red[11];
  if (tid == 0) {
    const float ce = valid ? row_loss(lse, xlab, bsx, o) : 0.f;
    loss_row[row] = valid ? kd_row_loss(ce, r.kl, kd) : 0.f;
    kl_row[row] = valid ? r.kl : 0.f;
  }
  if (!write_grad) return;
  const GradCoef q = grad_coef(lse, g, o);
  const bool live = g != 0.f;
  const float c2 = kd.alpha * (g * kd.T);
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int c = (it * 256 + tid) * VEC;
    if (c < V) {
      VT out;
#pragma unroll
      for (int u = 0; u < VEC; ++u) {
        const float xv = to_f32(v[it][u]), e = __expf(xv - lse);
        out[u] = from_f32<T>(kd_join<TEMP>(ce_elem(e, q), e, xv, tv[it].get(u), r, kd, c2, live));
      }
      const unsigned at = (unsigned)(labi - c);
      if (at < (unsigned)VEC) {
#pragma unroll
        for (int u = 0; u < VEC; ++u)
          if (u == (int)at) {
            const float xv = to_f32(v[it][u]), e = __expf(xv - lse);
            out[u] = from_f32<T>(kd_join<TEMP>(grad_at_label(e, q, o), e, xv, tv[it].get(u), r, kd, c2, live));
          }
      }
      *reinterpret_cast<VT*>(x + c) = out;
    }
  }
}

// ---- the launches ----------------------------------------------------------------------------------------------------------------
template <bool SX> struct Plain {
  template <int NIT> static constexpr auto onepass = ce_onepass_kernel<bf16_t, NIT, SX>;
  template <typename T> static constexpr auto twopass = ce_kernel<T, SX>;
};
template <typename TT, bool SX, bool TEMP> struct Distill {
  template <int NIT> static constexpr auto onepass = ce_kd_onepass_kernel<TT, NIT, SX, TEMP>;
  template <typename T> static constexpr auto twopass = ce_kd_kernel<T, TT, SX, TEMP>;
};
// the one dispatch on the student's dtype and width, for either kernel pair K: one-pass NIT 16 for 16384 < V <= 32768 bf16, NIT 8
// below, two-pass above and for f32.  args: the kernel's arguments behind the logits pointer
template <typename K, typename... A>
void launch_rows(hipStream_t s, int rows, int dtype, int V, void* logits, A... args) {
  const dim3 grid(rows), block(256);
  if (dtype == KLAB_BF16 && V <= 256 * 8 * 16 && V > 256 * 8 * 8)
    hipLaunchKernelGGL((K::template onepass<16>), grid, block, 0, s, (bf16_t*)logits, args...);
  else if (dtype == KLAB_BF16 && V <= 256 * 8 * 8)
    hipLaunchKernelGGL((K::template onepass<8>), grid, block, 0, s, (bf16_t*)logits, args...);
  else if (dtype == KLAB_BF16)
    hipLaunchKernelGGL((K::template twopass<bf16_t>), grid, block, 0, s, (bf16_t*)logits, args...);
  else
    hipLaunchKernelGGL((K::template twopass<float>), grid, block, 0, s, (float*)logits, args...);
}

// the three launches of every entry point: the norm (unless bit 1 of write_grad says that inv_w already holds it), the rows
// (rows_fn(write_grad & 1)), the reduce
template <typename F>
int ce_forward(const long long* labels, const float* weights, int rows, float* inv_w, float* loss_row, float* loss, int write_grad,
               hipStream_t s, F rows_fn) {
  if (!(write_grad & 2)) {
    hipLaunchKernelGGL(ce_norm_kernel, dim3(1), dim3(256), 0, s, labels, weights, rows, inv_w);
    KLAB_LAUNCH_CHECK();
  }
  rows_fn(write_grad & 1);
  KLAB_LAUNCH_CHECK();
  hipLaunchKernelGGL(ce_reduce_kernel, dim3(1), dim3(256), 0, s, loss_row, weights, rows, inv_w, loss);
  KLAB_LAUNCH_CHECK();
  return KLAB_OK;
}

// the cross-entropy without a teacher; sx: eps != 0
int ce_plain(void* logits, long ld, int dtype, const long long* labels, const float* weights, int rows, int V, CeOpts o, bool sx,
             float* inv_w, float* loss_row, float* loss, int write_grad, hipStream_t s) {
  return ce_forward(labels, weights, rows, inv_w, loss_row, loss, write_grad, s, [&](int wg) {
    const float* inv = inv_w;
    if (sx) launch_rows<Plain<true>>(s, rows, dtype, V, logits, ld, labels, weights, V, o, inv, loss_row, wg);
    else launch_rows<Plain<false>>(s, rows, dtype, V, logits, ld, labels, weights, V, o, inv, loss_row, wg);
  });
}

}  // namespace
}  // namespace klab

using namespace klab;

extern "C" int klab_ce_wsum(const long long* labels, const float* weights, int rows, float* inv_w, void* stream) {
  if (!labels || !inv_w || rows <= 0) return KLAB_ERR_BADARG;
  hipLaunchKernelGGL(ce_norm_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, labels, weights, rows, inv_w);
  KLAB_LAUNCH_CHECK();
  return KLAB_OK;
}

// inv_n[0] = 1 / (number of labels != -100): the first launch of klab_ce_fwd on its own, for callers that know the labels long before
// the logits exist (the engine runs it beside the Swin tower and passes write_grad | 2)
extern "C" int klab_ce_count(const long long* labels, int rows, float* inv_n, void* stream) { return klab_ce_wsum(labels, NULL, rows, inv_n, stream); }

extern "C" int klab_ce_fwd(void* logits, long ld, int dtype, const long long* labels, int rows, int V, float* inv_n, float* loss_row,
                           float* loss, int write_grad, void* stream) {
  if (!logits || !labels || !inv_n || !loss_row || !loss) return KLAB_ERR_BADARG;
  const int vec = dtype == KLAB_BF16 ? 8 : 4;
  if (V % vec || ld % vec) return KLAB_ERR_UNSUPPORTED;
  return ce_plain(logits, ld, dtype, labels, NULL, rows, V, CeOpts{1.f, 0.f, 0.f}, false, inv_n, loss_row, loss, write_grad, (hipStream_t)stream);
}

extern "C" int klab_ce_fwd_opts(void* logits, long ld, int dtype, const long long* labels, const float* weights, int rows, int V, float eps,
                                float z, float* inv_w, float* loss_row, float* loss, int write_grad, void* stream) {
  if (!logits || !labels || !inv_w || !loss_row || !loss || rows <= 0 || V <= 0) return KLAB_ERR_BADARG;
  if (!(eps >= 0.f && eps < 1.f) || !(z >= 0.f) || !isfinite(z)) return KLAB_ERR_BADARG;
  const int vec = dtype == KLAB_BF16 ? 8 : 4;
  if (V % vec || ld % vec) return KLAB_ERR_UNSUPPORTED;
  return ce_plain(logits, ld, dtype, labels, weights, rows, V, CeOpts{1.f - eps, eps / (float)V, z}, eps != 0.f, inv_w, loss_row, loss,
                  write_grad, (hipStream_t)stream);
}

extern "C" int klab_ce_fwd_distill(void* logits, long ld, int dtype, const void* teacher, long ldt, int t_dtype, const long long* labels,
                                   const float* weights, int rows, int V, float eps, float z, float alpha, float temperature, float* inv_w,
                                   float* loss_row, float* kl_row, float* loss, int write_grad, void* stream) {
  if (!logits || !teacher || !labels || !inv_w || !loss_row || !kl_row || !loss || rows <= 0 || V <= 0) return KLAB_ERR_BADARG;
  if (!(eps >= 0.f && eps < 1.f) || !(z >= 0.f) || !isfinite(z)) return KLAB_ERR_BADARG;
  if (!(alpha >= 0.f && alpha <= 1.f) || !(temperature > 0.f) || !isfinite(temperature)) return KLAB_ERR_BADARG;
  if (t_dtype != KLAB_BF16 && t_dtype != KLAB_F32) return KLAB_ERR_BADARG;
  const int vec = dtype == KLAB_BF16 ? 8 : 4, tvec = t_dtype == KLAB_BF16 ? 8 : 4;
  if (V % vec || ld % vec || V % tvec || ldt % tvec) return KLAB_ERR_UNSUPPORTED;
  if (ld < V || ldt < V) return KLAB_ERR_BADARG;
  {  // the teacher is read while the logits are rewritten: the two ranges must not meet
    const uintptr_t x0 = (uintptr_t)logits, x1 = x0 + ((size_t)(rows - 1) * ld + V) * (dtype == KLAB_BF16 ? 2 : 4);
    const uintptr_t t0 = (uintptr_t)teacher, t1 = t0 + ((size_t)(rows - 1) * ldt + V) * (t_dtype == KLAB_BF16 ? 2 : 4);
    if (x0 < t1 && t0 < x1) return KLAB_ERR_BADARG;
  }
  hipStream_t s = (hipStream_t)stream;
  const CeOpts o{1.f - eps, eps / (float)V, z};
  const KdOpts kd{alpha, 1.f - alpha, temperature, 1.f / temperature, alpha * (temperature * temperature)};
  const bool sx = eps != 0.f, temp = temperature != 1.f;
  return ce_forward(labels, weights, rows, inv_w, loss_row, loss, write_grad, s, [&](int wg) {
    auto go = [&](auto pair, auto* t) {
      launch_rows<decltype(pair)>(s, rows, dtype, V, logits, ld, t, ldt, labels, weights, V, o, kd, (const float*)inv_w, loss_row, kl_row, wg);
    };
    auto by_flags = [&](auto* t) {
      using TT = std::remove_cv_t<std::remove_pointer_t<decltype(t)>>;
      if (sx) temp ? go(Distill<TT, true, true>{}, t) : go(Distill<TT, true, false>{}, t);
      else temp ? go(Distill<TT, false, true>{}, t) : go(Distill<TT, false, false>{}, t);
    };
    if (t_dtype == KLAB_BF16) by_flags((const bf16_t*)teacher);
    else by_flags((const float*)teacher);
  });
}
