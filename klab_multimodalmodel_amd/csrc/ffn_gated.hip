// Gate of the T5 v1.1 / Flan-T5 feed-forward (HF T5DenseGatedActDense): h = dropout(gelu_new(wi_0 x) * (wi_1 x)).
// The two projections run as ONE GEMM with N = 2F whose output ab [M, 2F] keeps a = ab[:, :F] and b = ab[:, F:] side by side; the
// kernels here are the element-wise pass between that product and wo (forward), and between wo's dgrad and the K = 2F dgrad
// (backward).  Streaming kernels: one 16-byte vector of a, b (and dh) per thread per step, one (two) 16-byte stores, f32 arithmetic.
// The dropout mask is keep(seed, tag, m * F + f), regenerated in backward; a and b are what backward needs, h feeds wo's wgrad.
#include "common.h"
#include "klab_mm.h"

namespace {
using namespace klab;

constexpr float kC0 = 0.7978845608028654f;  // sqrt(2 / pi)
constexpr float kC1 = 0.044715f;

// tanh of the gelu_new argument.  bf16 engines: 1 - 2 / (exp(2u) + 1) on v_exp_f32 (absolute error ~1e-7, far below the bf16
// rounding of the result; saturates correctly: exp -> inf gives 1, exp -> 0 gives -1).  fp32 parity engines: libm tanhf.
template <typename T> __device__ __forceinline__ float tanh_for(float u) {
  if constexpr (sizeof(T) == 2) return 1.f - 2.f * __frcp_rn(__expf(2.f * u) + 1.f);
  else return tanhf(u);
}
// gelu_new(x) = 0.5 x (1 + tanh(c0 (x + c1 x^3))) and its derivative
template <typename T> __device__ __forceinline__ void gelu_new_both(float x, float& g, float& dg) {
  // x^2 is capped: beyond |x| = 1e4 the tanh is +-1 either way, and an infinite x^2 (|x| >= 1.85e19) made the derivative's
  // polynomial infinite against a factor (1 - t^2) = 0: NaN for a finite input
  const float x2 = fminf(x * x, 1e8f);
  const float t = tanh_for<T>(kC0 * x * fmaf(kC1, x2, 1.f));
  const float hp = 0.5f * (1.f + t);
  g = x * hp;
  dg = fmaf(0.5f * x * (1.f - t * t), kC0 * fmaf(3.f * kC1, x2, 1.f), hp);
}
template <typename T> __device__ __forceinline__ float gelu_new_val(float x) {
  const float t = tanh_for<T>(kC0 * x * fmaf(kC1, x * x, 1.f));
  return 0.5f * x * (1.f + t);
}

template <typename T>
__global__ __launch_bounds__(256) void geglu_fwd_kernel(const T* __restrict__ ab, long ldab, T* __restrict__ h, long ldh, int M, int F, float p,
                                                        const uint32_t* __restrict__ seed_dev, uint32_t tag) {
  typedef typename Vec16<T>::type V;
  constexpr int N = Vec16<T>::N;
  const DropCtx dc = make_drop(seed_dev, tag, p);
  const int fv = F / N;
  const long total = (long)M * fv;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long m = i / fv;
    const int f = (int)(i - m * fv) * N;
    const V a = *reinterpret_cast<const V*>(ab + m * ldab + f);
    const V b = *reinterpret_cast<const V*>(ab + m * ldab + F + f);
    V o;
#pragma unroll
    for (int e = 0; e < N; ++e) {
      const float v = gelu_new_val<T>(to_f32(a[e])) * to_f32(b[e]);
      o[e] = from_f32<T>(v * drop_mult(dc, (uint64_t)m * (uint64_t)F + (uint64_t)(f + e)));
    }
    *reinterpret_cast<V*>(h + m * ldh + f) = o;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void geglu_bwd_kernel(const T* __restrict__ dh, long lddh, const T* __restrict__ ab, long ldab,
                                                        T* __restrict__ dab, long lddab, int M, int F, float p,
                                                        const uint32_t* __restrict__ seed_dev, uint32_t tag) {
  typedef typename Vec16<T>::type V;
  constexpr int N = Vec16<T>::N;
  const DropCtx dc = make_drop(seed_dev, tag, p);
  const int fv = F / N;
  const long total = (long)M * fv;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long m = i / fv;
    const int f = (int)(i - m * fv) * N;
    const V g = *reinterpret_cast<const V*>(dh + m * lddh + f);
    const V a = *reinterpret_cast<const V*>(ab + m * ldab + f);
    const V b = *reinterpret_cast<const V*>(ab + m * ldab + F + f);
    V da, db;
#pragma unroll
    for (int e = 0; e < N; ++e) {
      float ga, dga;
      gelu_new_both<T>(to_f32(a[e]), ga, dga);
      const float gm = to_f32(g[e]) * drop_mult(dc, (uint64_t)m * (uint64_t)F + (uint64_t)(f + e));
      da[e] = from_f32<T>(gm * to_f32(b[e]) * dga);
      db[e] = from_f32<T>(gm * ga);
    }
    *reinterpret_cast<V*>(dab + m * lddab + f) = da;
    *reinterpret_cast<V*>(dab + m * lddab + F + f) = db;
  }
}

inline unsigned stream_grid(long work_items) {
  long g = (work_items + 255) / 256;
  if (g < 1) g = 1;
  if (g > 2048) g = 2048;  // cap + grid-stride (memory-bound grid sizing rule)
  return (unsigned)g;
}
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int klab_geglu_fwd(const void* ab, long ldab, void* h, long ldh, int dtype, int M, int F, float drop_p, const uint32_t* seed_dev,
                              uint32_t drop_tag, void* stream) {
  if (!ab || !h || M < 0 || F <= 0 || ldab < 2L * F || ldh < F || drop_p < 0.f || drop_p >= 1.f || (drop_p > 0.f && !seed_dev))
    return KLAB_ERR_BADARG;
  if (dtype != KLAB_F32 && dtype != KLAB_BF16) return KLAB_ERR_BADARG;
  if ((F & 7) || (ldab & 7) || (ldh & 7) || !aligned16(ab) || !aligned16(h)) return KLAB_ERR_UNSUPPORTED;
  if (M == 0) return KLAB_OK;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == KLAB_BF16)
    hipLaunchKernelGGL(geglu_fwd_kernel<bf16_t>, dim3(stream_grid((long)M * F / 8)), dim3(256), 0, s, (const bf16_t*)ab, ldab, (bf16_t*)h, ldh, M,
                       F, drop_p, seed_dev, drop_tag);
  else
    hipLaunchKernelGGL(geglu_fwd_kernel<float>, dim3(stream_grid((long)M * F / 4)), dim3(256), 0, s, (const float*)ab, ldab, (float*)h, ldh, M, F,
                       drop_p, seed_dev, drop_tag);
  KLAB_LAUNCH_CHECK();
  return KLAB_OK;
}

extern "C" int klab_geglu_bwd(const void* dh, long lddh, const void* ab, long ldab, void* dab, long lddab, int dtype, int M, int F, float drop_p,
                              const uint32_t* seed_dev, uint32_t drop_tag, void* stream) {
  if (!dh || !ab || !dab || M < 0 || F <= 0 || lddh < F || ldab < 2L * F || lddab < 2L * F || drop_p < 0.f || drop_p >= 1.f ||
      (drop_p > 0.f && !seed_dev))
    return KLAB_ERR_BADARG;
  if (dtype != KLAB_F32 && dtype != KLAB_BF16) return KLAB_ERR_BADARG;
  if ((F & 7) || (lddh & 7) || (ldab & 7) || (lddab & 7) || !aligned16(dh) || !aligned16(ab) || !aligned16(dab)) return KLAB_ERR_UNSUPPORTED;
  if (M == 0) return KLAB_OK;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == KLAB_BF16)
    hipLaunchKernelGGL(geglu_bwd_kernel<bf16_t>, dim3(stream_grid((long)M * F / 8)), dim3(256), 0, s, (const bf16_t*)dh, lddh, (const bf16_t*)ab,
                       ldab, (bf16_t*)dab, lddab, M, F, drop_p, seed_dev, drop_tag);
  else
    hipLaunchKernelGGL(geglu_bwd_kernel<float>, dim3(stream_grid((long)M * F / 4)), dim3(256), 0, s, (const float*)dh, lddh, (const float*)ab, ldab,
                       (float*)dab, lddab, M, F, drop_p, seed_dev, drop_tag);
  KLAB_LAUNCH_CHECK();
  return KLAB_OK;
}
