// LM-head cross-entropy with knowledge distillation: the loss of ce_opts.hip mixed with the KL divergence from a teacher's logits
// t [rows, V] (read-only, bf16 or f32, its own row stride) at temperature T, in the same pass over the student's row.
//
//   ce      = lse(x) - (1 - eps) x_y - (eps / V) sum_j x_j + z lse(x)^2                      (ce_opts.hip's l)
//   p       = softmax(t / T),  q = softmax(x / T)
//   kl      = sum_j p_j (log p_j - log q_j) = (1 / T) (sum_j p_j (t_j - x_j) - (max t - max x)) - log st + log sq
//             with st = sum_j exp((t_j - max t) / T), sq = sum_j exp((x_j - max x) / T)
//   l       = (1 - alpha) ce + alpha T^2 kl                                                   (0 where y == -100)
//   loss    = sum_i w_i l_i / W
//   dl/dx_j = (w_i / W) [ (1 - alpha) (softmax(x)_j (1 + 2 z lse) - (1 - eps) delta_jy - eps / V) + alpha T (q_j - p_j) ]
//
// Forms and byte traffic are ce_opts.hip's with the teacher's row beside the student's: register-resident one-pass for bf16
// student rows up to 32768 logits (student read once and written once, teacher read once), two-pass (online soft-max) above that
// and for f32 student logits.  Exponentials per logit: 4 at T == 1 (exp(x - max), exp(t - max) for the sums; exp(x - lse),
// exp(t - lse_t) for the gradient -- q is softmax(x) there and sq the cross-entropy's sum), 6 otherwise (exp((x - max) / T) and
// q_j on top); the plain and the options kernel have 2.
//
// alpha == 0 gives the bits of klab_ce_fwd_opts: the cross-entropy part is computed by the same operations in the same order and
// joins as (1 - alpha) a + alpha b, where 1 - alpha = 1 and alpha b = 0 (the teacher is finite).  A row with g = w / W == 0 takes
// the cross-entropy's value alone, so that the sign of its zeros is ce_opts.hip's too.  With a teacher equal to the student's
// logits the large terms vanish instead of cancelling: t_j - x_j = 0 and the maxima agree, which leaves log sq - log st, two sums
// of the same values.
#include <math.h>
#include <stdint.h>

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

// ---- the cross-entropy part: ce_opts.hip's expressions, operation for operation ------------------------------------------------
__device__ __forceinline__ float row_loss(float lse, float xlab, float sx, const CeOpts& o) {
  float l = lse - o.ome * xlab;
  l -= o.epsv * sx;
  l += (o.z * lse) * lse;
  return l;
}
struct GradCoef {
  float gk, ge, k, g;
};
__device__ __forceinline__ GradCoef grad_coef(float lse, float g, const CeOpts& o) {
  const float k = 1.f + 2.f * (o.z * lse);
  return GradCoef{g * k, g * o.epsv, k, g};
}
// The two multiply-adds are spelled out: ce_opts.hip's `p * gk - ge` and `p * k - (1 - eps)` compile to one fused instruction each
// in every one of its kernels, and beside the distillation term the compiler's contraction of the same source expression is no
// longer uniform (it left half of the f32 kernel's elements unfused, one unit in the last place off ce_opts.hip's).
__device__ __forceinline__ float ce_elem(float pr, const GradCoef& q) { return __builtin_fmaf(pr, q.gk, -q.ge); }
__device__ __forceinline__ float grad_at_label(float pr, const GradCoef& q, const CeOpts& o) {
  float t = __builtin_fmaf(pr, q.k, -o.ome);
  t -= o.epsv;
  return t * q.g;
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
    r.kl = ((s - (tm - bm)) * k.invT - lst) + lsq;
    r.lqT = bm * k.invT + lsq;
    r.ltT = tm * k.invT + lst;
  } else {
    r.kl = ((s - (tm - bm)) - lst) + lsq;
    r.lqT = r.lse;
    r.ltT = tm + lst;
  }
  return r;
}

// one element of the gradient.  a: the cross-entropy's element (ce_opts.hip's), e = exp(x - lse)
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

// ---- two-pass form: online soft-max of both rows, then the gradient ---------------------------------------------------------------
template <typename T, typename TT, bool SX, bool TEMP>
__global__ __launch_bounds__(256) void ce_distill_kernel(T* __restrict__ logits, long ld, const TT* __restrict__ teacher, long ldt,
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
  float m = -INFINITY, s = 0.f, sx = 0.f;        // the cross-entropy's (ce_opts_kernel)
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
    loss_row[row] = valid ? kd.oma * ce + kd.aT2 * r.kl : 0.f;
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

// ---- one-pass form (ce_opts_onepass_kernel with the teacher's row beside the student's): every load of both rows is issued
// before the first use, d logits leave the registers -------------------------------------------------------------------------------
template <typename TT, int NIT, bool SX, bool TEMP>
__global__ __launch_bounds__(256) void ce_distill_onepass_kernel(bf16_t* __restrict__ logits, long ld, const TT* __restrict__ teacher, long ldt,
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
    loss_row[row] = valid ? kd.oma * ce + kd.aT2 * r.kl : 0.f;
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

// loss[0] = (sum_i w_i l_i) inv_w: ce_opts.hip's ce_wreduce_kernel, operation for operation
__global__ __launch_bounds__(256) void ce_distill_reduce_kernel(const float* __restrict__ loss_row, const float* __restrict__ weights, int rows,
                                                                const float* __restrict__ inv_w, float* __restrict__ loss) {
  __shared__ float red[4];
  float a = 0.f;
  for (int i = threadIdx.x; i < rows; i += 256) a += weights ? weights[i] * loss_row[i] : loss_row[i];  // fixed order => bit-reproducible
  a = wave_sum(a);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) loss[0] = (red[0] + red[1] + red[2] + red[3]) * inv_w[0];
}

struct RowArgs {
  void* logits; long ld; int dtype;
  const void* teacher; long ldt;
  const long long* labels; const float* weights; int rows, V;
  CeOpts o; KdOpts kd;
  const float* inv_w; float* loss_row; float* kl_row; int write_grad;
  hipStream_t s;
};

// ce_opts.hip's dispatch on the student's dtype and width
template <typename TT, bool SX, bool TEMP>
void launch_rows(const RowArgs& a) {
  const dim3 grid(a.rows), block(256);
  const TT* t = (const TT*)a.teacher;
  if (a.dtype == KLAB_BF16 && a.V <= 256 * 8 * 16 && a.V > 256 * 8 * 8)
    hipLaunchKernelGGL((ce_distill_onepass_kernel<TT, 16, SX, TEMP>), grid, block, 0, a.s, (bf16_t*)a.logits, a.ld, t, a.ldt, a.labels, a.weights, a.V,
                       a.o, a.kd, a.inv_w, a.loss_row, a.kl_row, a.write_grad);
  else if (a.dtype == KLAB_BF16 && a.V <= 256 * 8 * 8)
    hipLaunchKernelGGL((ce_distill_onepass_kernel<TT, 8, SX, TEMP>), grid, block, 0, a.s, (bf16_t*)a.logits, a.ld, t, a.ldt, a.labels, a.weights, a.V,
                       a.o, a.kd, a.inv_w, a.loss_row, a.kl_row, a.write_grad);
  else if (a.dtype == KLAB_BF16)
    hipLaunchKernelGGL((ce_distill_kernel<bf16_t, TT, SX, TEMP>), grid, block, 0, a.s, (bf16_t*)a.logits, a.ld, t, a.ldt, a.labels, a.weights, a.V,
                       a.o, a.kd, a.inv_w, a.loss_row, a.kl_row, a.write_grad);
  else
    hipLaunchKernelGGL((ce_distill_kernel<float, TT, SX, TEMP>), grid, block, 0, a.s, (float*)a.logits, a.ld, t, a.ldt, a.labels, a.weights, a.V,
                       a.o, a.kd, a.inv_w, a.loss_row, a.kl_row, a.write_grad);
}
template <typename TT>
void launch_teacher(const RowArgs& a, bool sx, bool temp) {
  if (sx) temp ? launch_rows<TT, true, true>(a) : launch_rows<TT, true, false>(a);
  else temp ? launch_rows<TT, false, true>(a) : launch_rows<TT, false, false>(a);
}

}  // namespace
}  // namespace klab

using namespace klab;

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
  if (!(write_grad & 2)) {  // bit 1: inv_w already holds 1 / W of these labels and weights (klab_ce_wsum)
    const int rc = klab_ce_wsum(labels, weights, rows, inv_w, stream);
    if (rc != KLAB_OK) return rc;
  }
  RowArgs a{logits, ld, dtype, teacher, ldt, labels, weights, rows, V, CeOpts{1.f - eps, eps / (float)V, z},
            KdOpts{alpha, 1.f - alpha, temperature, 1.f / temperature, alpha * (temperature * temperature)}, inv_w, loss_row, kl_row,
            write_grad & 1, s};
  const bool temp = temperature != 1.f;
  if (t_dtype == KLAB_BF16) launch_teacher<bf16_t>(a, eps != 0.f, temp);
  else launch_teacher<float>(a, eps != 0.f, temp);
  KLAB_LAUNCH_CHECK();
  hipLaunchKernelGGL(ce_distill_reduce_kernel, dim3(1), dim3(256), 0, s, loss_row, weights, rows, inv_w, loss);
  KLAB_LAUNCH_CHECK();
  return KLAB_OK;
}
