// LM-head cross-entropy with options: label smoothing eps, z-loss z and per-row weights w (all three optional), beside the plain
// kernels of misc.hip, which stay the path of a model that sets none of them.
//
//   l_i     = lse - (1 - eps) x_y - (eps / V) sum_j x_j + z lse^2        (0 where y == -100)
//   loss    = sum_i w_i l_i / W,   W = sum_{i : y_i != -100} w_i          (0 when W == 0)
//   dl/dx_j = (w_i / W) [ p_j (1 + 2 z lse) - (1 - eps) delta_jy - eps / V ]
//
// The two forms of the plain kernel are kept with their byte traffic: the register-resident one-pass form for bf16 rows up to
// 32768 logits (the row is read once) and the two-pass form above that and for f32.  The extra work of a row is one weight load
// and, with eps != 0, one more accumulator (sum_j x_j) in the pass that exists anyway.
//
// Neutral options (eps = 0, z = 0, weights NULL or all ones) give the bits of klab_ce_fwd: lse is computed by the same operations
// in the same order, and every added operation is then exact -- 1 - eps = 1, eps / V = 0, z lse = 0, 1 + 2 z lse = 1 and
// w inv_w = inv_n -- so each expression below rounds once where the plain kernel's rounds once, fused or not.
#include <math.h>

#include "common.h"
#include "klab_mm.h"

namespace klab {
namespace {

struct CeOpts {
  float ome;   // 1 - eps
  float epsv;  // eps / V
  float z;
};

// inv_w[0] = 1 / sum of the weights of the rows with a label, 0 when that sum is 0.  One workgroup, fixed order.  Weights of all
// ones (or NULL) sum to the exact count (< 2^24), so the quotient is ce_count_kernel's.
__global__ __launch_bounds__(256) void ce_wsum_kernel(const long long* __restrict__ labels, const float* __restrict__ weights, int rows,
                                                      float* __restrict__ inv_w) {
  __shared__ float red[4];
  float a = 0.f;
  for (int i = threadIdx.x; i < rows; i += 256) a += labels[i] != -100 ? (weights ? weights[i] : 1.f) : 0.f;
  a = wave_sum(a);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float W = red[0] + red[1] + red[2] + red[3];
    inv_w[0] = W > 0.f ? 1.f / W : 0.f;
  }
}

__device__ __forceinline__ float row_loss(float lse, float xlab, float sx, const CeOpts& o) {
  float l = lse - o.ome * xlab;
  l -= o.epsv * sx;
  l += (o.z * lse) * lse;
  return l;
}

// The gradient of a row is g [p_j k - (1 - eps) delta_jy - eps / V] with g = w inv_w and k = 1 + 2 z lse.  Off the label that is
// ONE fused multiply-add per element, p_j (g k) - g eps / V -- the plain kernel's p_j g when the options are neutral, and exact
// zeros when g == 0 -- and the label's element is mended afterwards by the one lane that holds it, as ((p_y k - (1 - eps)) - eps / V) g:
// (p_y - 1) g with neutral options, the plain kernel's two roundings.  Both kernels are VALU-bound next to their two __expf per
// logit, so the label is looked for once per 16-byte vector, not once per element.
struct GradCoef {
  float gk, ge, k, g;
};
__device__ __forceinline__ GradCoef grad_coef(float lse, float g, const CeOpts& o) {
  const float k = 1.f + 2.f * (o.z * lse);
  return GradCoef{g * k, g * o.epsv, k, g};
}
__device__ __forceinline__ float grad_at_label(float pr, const GradCoef& q, const CeOpts& o) {
  float t = pr * q.k - o.ome;
  t -= o.epsv;
  return t * q.g;
}

// SX: the row sum of the logits is wanted (eps != 0); without it the first pass is the plain kernel's
template <typename T, bool SX>
__global__ __launch_bounds__(256) void ce_opts_kernel(T* __restrict__ logits, long ld, const long long* __restrict__ labels,
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
    for (int u = 0; u < VEC; ++u) out[u] = from_f32<T>(__expf(to_f32(v[u]) - lse) * q.gk - q.ge);
    const unsigned at = (unsigned)(labi - c);
    if (at < (unsigned)VEC) {
#pragma unroll
      for (int u = 0; u < VEC; ++u)
        if (u == (int)at) out[u] = from_f32<T>(grad_at_label(__expf(to_f32(v[u]) - lse), q, o));
    }
    *reinterpret_cast<VT*>(x + c) = out;
  }
}

// the one-pass form (see ce_fwd_onepass_kernel): every load of the row is issued before the first use, d logits leave the registers
template <typename T, int NIT, bool SX>
__global__ __launch_bounds__(256) void ce_opts_onepass_kernel(T* __restrict__ logits, long ld, const long long* __restrict__ labels,
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
      for (int u = 0; u < VEC; ++u) out[u] = from_f32<T>(__expf(to_f32(v[it][u]) - lse) * q.gk - q.ge);
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

// loss[0] = (sum_i w_i l_i) inv_w in ce_reduce_kernel's order (rows without a label hold l = 0)
__global__ __launch_bounds__(256) void ce_wreduce_kernel(const float* __restrict__ loss_row, const float* __restrict__ weights, int rows,
                                                         const float* __restrict__ inv_w, float* __restrict__ loss) {
  __shared__ float red[4];
  float a = 0.f;
  for (int i = threadIdx.x; i < rows; i += 256) a += weights ? weights[i] * loss_row[i] : loss_row[i];  // fixed order => bit-reproducible
  a = wave_sum(a);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) loss[0] = (red[0] + red[1] + red[2] + red[3]) * inv_w[0];
}

// the plain kernel's dispatch; SX: the row sum of the logits is needed (eps != 0)
template <bool SX>
void launch_rows(void* logits, long ld, int dtype, const long long* labels, const float* weights, int rows, int V, const CeOpts& o,
                 const float* inv_w, float* loss_row, int write_grad, hipStream_t s) {
  if (dtype == KLAB_BF16 && V <= 256 * 8 * 16 && V > 256 * 8 * 8)
    hipLaunchKernelGGL((ce_opts_onepass_kernel<bf16_t, 16, SX>), dim3(rows), dim3(256), 0, s, (bf16_t*)logits, ld, labels, weights, V, o, inv_w, loss_row, write_grad);
  else if (dtype == KLAB_BF16 && V <= 256 * 8 * 8)
    hipLaunchKernelGGL((ce_opts_onepass_kernel<bf16_t, 8, SX>), dim3(rows), dim3(256), 0, s, (bf16_t*)logits, ld, labels, weights, V, o, inv_w, loss_row, write_grad);
  else if (dtype == KLAB_BF16)
    hipLaunchKernelGGL((ce_opts_kernel<bf16_t, SX>), dim3(rows), dim3(256), 0, s, (bf16_t*)logits, ld, labels, weights, V, o, inv_w, loss_row, write_grad);
  else
    hipLaunchKernelGGL((ce_opts_kernel<float, SX>), dim3(rows), dim3(256), 0, s, (float*)logits, ld, labels, weights, V, o, inv_w, loss_row, write_grad);
}

}  // namespace
}  // namespace klab

using namespace klab;

extern "C" int klab_ce_wsum(const long long* labels, const float* weights, int rows, float* inv_w, void* stream) {
  if (!labels || !inv_w || rows <= 0) return KLAB_ERR_BADARG;
  hipLaunchKernelGGL(ce_wsum_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, labels, weights, rows, inv_w);
  KLAB_LAUNCH_CHECK();
  return KLAB_OK;
}

extern "C" int klab_ce_fwd_opts(void* logits, long ld, int dtype, const long long* labels, const float* weights, int rows, int V, float eps,
                                float z, float* inv_w, float* loss_row, float* loss, int write_grad, void* stream) {
  if (!logits || !labels || !inv_w || !loss_row || !loss || rows <= 0 || V <= 0) return KLAB_ERR_BADARG;
  if (!(eps >= 0.f && eps < 1.f) || !(z >= 0.f) || !isfinite(z)) return KLAB_ERR_BADARG;
  const int vec = dtype == KLAB_BF16 ? 8 : 4;
  if (V % vec || ld % vec) return KLAB_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  if (!(write_grad & 2)) {  // bit 1: inv_w already holds 1 / W of these labels and weights (klab_ce_wsum)
    hipLaunchKernelGGL(ce_wsum_kernel, dim3(1), dim3(256), 0, s, labels, weights, rows, inv_w);
    KLAB_LAUNCH_CHECK();
  }
  write_grad &= 1;
  const CeOpts o{1.f - eps, eps / (float)V, z};
  if (eps != 0.f) launch_rows<true>(logits, ld, dtype, labels, weights, rows, V, o, inv_w, loss_row, write_grad, s);
  else launch_rows<false>(logits, ld, dtype, labels, weights, rows, V, o, inv_w, loss_row, write_grad, s);
  KLAB_LAUNCH_CHECK();
  hipLaunchKernelGGL(ce_wreduce_kernel, dim3(1), dim3(256), 0, s, loss_row, weights, rows, inv_w, loss);
  KLAB_LAUNCH_CHECK();
  return KLAB_OK;
}
