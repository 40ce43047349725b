// Fused multi-tensor Adam (math of torch.optim.Adam, L2 decay folded into the gradient; SURVEY 8 f-2, ref/train.py:28) and AdamW
// (decoupled weight decay; torch.optim.AdamW's single-tensor rule without amsgrad / maximize, with per-GROUP hyper-parameters),
// both with the compute-dtype shadow copy: the separate cast pass over the masters disappears.
//
// One pass over the trainable tensors, whatever the number of parameter groups: p, g, m, v in as 16-byte non-temporal vectors,
// p, m, v out, and -- for tensors with aoff >= 0 -- the bf16 / f32 copy the next forward's GEMMs read, straight into the weight
// arena.  30 bytes per parameter.  m / v live in flat buffers laid out like the flat gradient buffer.  The table walk and its
// launch shape are multi_tensor.h's; adam_load / adam_store below are what the two kernels share, their update rules stay apart (the
// roundings differ: Adam is not AdamW with one group).
//
// AdamW's tables.  A second device table, group_of[nd] in the AdamDesc table's order, names each tensor's parameter group and
// goes to LDS with it.  The groups' hyper-parameters (at most KLAB_ADAMW_MAX_GROUPS) arrive BY VALUE in the kernel arguments,
// already derived on the host, and are copied to LDS once per workgroup: no host -> device copy per step, no device -> host
// read, and no global load in front of the streaming loads that depends on another.
//
// AdamW per element, in f32 and in this order (torch's order):
//   p'  = p * decay                               decay = (float)(1.0 - (double)lr * (double)weight_decay)
//   m'  = m + (1 - beta1) (g - m)
//   v'  = beta2 v + (1 - beta2) g^2
//   p'' = p' - step * (m' / (sqrt(v') * inv_sqrt_bc2 + eps))      step = (float)((double)lr / bias_corr1)
// lr = 0 gives decay = 1 and step = 0: p keeps its bits while m and v move on.
#include <math.h>

#include <type_traits>

#include "common.h"
#include "klab_mm.h"
#include "multi_tensor.h"

namespace klab {
namespace {

struct AdamHyper { float lr_over_bc1, beta1, beta2, eps, weight_decay, inv_sqrt_bc2; };
struct alignas(32) AdamWHyper { float decay, one_minus_beta1, beta2, one_minus_beta2, step, inv_sqrt_bc2, eps, pad; };
struct AdamWGroups { AdamWHyper g[KLAB_ADAMW_MAX_GROUPS]; };

static_assert((KLAB_ADAMW_MAX_GROUPS & (KLAB_ADAMW_MAX_GROUPS - 1)) == 0, "a group id is masked into the LDS table");

// What the two kernels share: the four streaming loads of one vec4 of p, g, m, v and where they came from (adam_load), and the
// stores of p', m', v' plus the compute-dtype copy of p' into the arena (adam_store).  The loop and its per-thread arrays stay
// in each kernel, on purpose: with the loop in a shared function, or the arrays in a struct, hipcc allocates 106-112 VGPRs (4
// waves per SIMD) instead of 172 (2), and that form of the step measured 302 us against 292.
__device__ __forceinline__ void adam_load(const AdamDesc& d, long local, const float* __restrict__ grads, const float* __restrict__ m,
                                          const float* __restrict__ v, float*& pp, long& go, long& ao, f32x4& pv, f32x4& gv, f32x4& mv, f32x4& vv) {
  pp = d.p + local; go = d.goff + local; ao = d.aoff < 0 ? -1 : d.aoff + local;
  pv = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(pp));
  gv = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(grads + go));
  mv = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(m + go));
  vv = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(v + go));
}
template <typename T>
__device__ __forceinline__ void adam_store(float* pp, long go, long ao, f32x4 po, f32x4 mo, f32x4 vo, float* __restrict__ m, float* __restrict__ v,
                                           T* __restrict__ arena) {
  __builtin_nontemporal_store(po, reinterpret_cast<f32x4*>(pp));
  __builtin_nontemporal_store(mo, reinterpret_cast<f32x4*>(m + go));
  __builtin_nontemporal_store(vo, reinterpret_cast<f32x4*>(v + go));
  if (ao >= 0) mt_store_vec4(arena + ao, po);
}

// vec4 indices [begin4, total4) of the table's prefix space (a sub-range = the tensors of one backward segment)
template <typename T, int U>
__global__ __launch_bounds__(256) void adam_step_kernel(const AdamDesc* __restrict__ dglob, int nd, long begin4, long total4, const float* __restrict__ grads,
                                                        float* __restrict__ m, float* __restrict__ v, T* __restrict__ arena, AdamHyper h) {
  __shared__ AdamDesc dsh[MT_MAXD];
  TableWalker<AdamDesc> w{mt_stage_table(dsh, dglob, nd), nd, 0};
  for (long g0 = begin4 + ((long)blockIdx.x * U) * blockDim.x + threadIdx.x; g0 < total4; g0 += (long)gridDim.x * U * blockDim.x) {
    w.seek(g0);
    f32x4 pv[U], gv[U], mv[U], vv[U];
    float* pp[U]; long go[U]; long ao[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long g = g0 + (long)u * blockDim.x;
      pp[u] = nullptr;
      if (g < total4) {
        const long local = w.advance(g);
        adam_load(w.cur(), local, grads, m, v, pp[u], go[u], ao[u], pv[u], gv[u], mv[u], vv[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (pp[u]) {
        f32x4 po, mo, vo;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float g = gv[u][i] + h.weight_decay * pv[u][i];
          mo[i] = mv[u][i] + (1.f - h.beta1) * (g - mv[u][i]);         // exp_avg.lerp_(grad, 1 - beta1)
          vo[i] = h.beta2 * vv[u][i] + (1.f - h.beta2) * g * g;        // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2)
          const float denom = sqrtf(vo[i]) * h.inv_sqrt_bc2 + h.eps;
          po[i] = pv[u][i] - h.lr_over_bc1 * (mo[i] / denom);
        }
        adam_store(pp[u], go[u], ao[u], po, mo, vo, m, v, arena);
      }
  }
}

template <typename T, int U>
__global__ __launch_bounds__(256) void adamw_step_kernel(const AdamDesc* __restrict__ dglob, int nd, const int* __restrict__ group_of,
                                                         long begin4, long total4, const float* __restrict__ grads, float* __restrict__ m,
                                                         float* __restrict__ v, T* __restrict__ arena, const AdamWGroups hy) {
  __shared__ AdamDesc dsh[MT_MAXD];
  __shared__ unsigned char gsh[MT_MAXD];  // (+ 1 KiB of group ids)
  __shared__ AdamWHyper hsh[KLAB_ADAMW_MAX_GROUPS];
  const bool in_lds = nd <= MT_MAXD;
  {
    constexpr int NW = (int)(sizeof(AdamWGroups) / sizeof(float));
    const float* src = reinterpret_cast<const float*>(&hy);
    float* dst = reinterpret_cast<float*>(hsh);
    for (int i = threadIdx.x; i < NW; i += blockDim.x) dst[i] = src[i];
  }
  if (in_lds)
    for (int i = threadIdx.x; i < nd; i += blockDim.x) gsh[i] = (unsigned char)group_of[i];
  TableWalker<AdamDesc> w{mt_stage_table(dsh, dglob, nd), nd, 0};  // (its barrier covers hsh and gsh)
  for (long g0 = begin4 + ((long)blockIdx.x * U) * blockDim.x + threadIdx.x; g0 < total4; g0 += (long)gridDim.x * U * blockDim.x) {
    w.seek(g0);
    f32x4 pv[U], gv[U], mv[U], vv[U];
    float* pp[U]; long go[U]; long ao[U]; int gi[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long g = g0 + (long)u * blockDim.x;
      pp[u] = nullptr;
      if (g < total4) {
        const long local = w.advance(g);
        // the group id is consumed only after the streaming loads below are in flight
        gi[u] = (in_lds ? (int)gsh[w.lo] : group_of[w.lo]) & (KLAB_ADAMW_MAX_GROUPS - 1);
        adam_load(w.cur(), local, grads, m, v, pp[u], go[u], ao[u], pv[u], gv[u], mv[u], vv[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (pp[u]) {
        const AdamWHyper h = hsh[gi[u]];
        f32x4 po, mo, vo;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float g = gv[u][i];
          const float pd = pv[u][i] * h.decay;                             // param.mul_(1 - lr * weight_decay)
          mo[i] = mv[u][i] + h.one_minus_beta1 * (g - mv[u][i]);          // exp_avg.lerp_(grad, 1 - beta1)
          vo[i] = h.beta2 * vv[u][i] + h.one_minus_beta2 * g * g;         // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2)
          const float denom = sqrtf(vo[i]) * h.inv_sqrt_bc2 + h.eps;
          po[i] = pd - h.step * (mo[i] / denom);
        }
        adam_store(pp[u], go[u], ao[u], po, mo, vo, m, v, arena);
      }
  }
}

}  // namespace
}  // namespace klab

using namespace klab;

extern "C" int klab_adam_step_range(const void* desc_dev, int ndesc, long begin4, long end4, const float* grads, float* m, float* v, void* arena,
                                    int dtype, float lr, float beta1, float beta2, float eps, float weight_decay, float bias_corr1,
                                    float bias_corr2, void* stream) {
  if (!desc_dev || ndesc <= 0 || !grads || !m || !v || !arena || bias_corr1 <= 0.f || bias_corr2 <= 0.f || begin4 < 0 || end4 < begin4)
    return KLAB_ERR_BADARG;
  if (end4 == begin4) return KLAB_OK;
  const AdamHyper h{lr / bias_corr1, beta1, beta2, eps, weight_decay, 1.f / sqrtf(bias_corr2)};
  mt_dispatch(dtype, arena, [&](auto* a) {
    hipLaunchKernelGGL((adam_step_kernel<std::remove_pointer_t<decltype(a)>, MT_U>), dim3(mt_grid(end4 - begin4)), dim3(256), 0, (hipStream_t)stream,
                       (const AdamDesc*)desc_dev, ndesc, begin4, end4, grads, m, v, a, h);
  });
  KLAB_LAUNCH_CHECK();
  return KLAB_OK;
}
extern "C" int klab_adam_step(const void* desc_dev, int ndesc, long total4, const float* grads, float* m, float* v, void* arena, int dtype,
                              float lr, float beta1, float beta2, float eps, float weight_decay, float bias_corr1, float bias_corr2,
                              void* stream) {
  return klab_adam_step_range(desc_dev, ndesc, 0, total4, grads, m, v, arena, dtype, lr, beta1, beta2, eps, weight_decay, bias_corr1, bias_corr2,
                              stream);
}

extern "C" int klab_adamw_step_range(const void* desc_dev, int ndesc, const int* group_of_dev, const klab_adamw_group* groups, int ngroups,
                                     long begin4, long end4, const float* grads, float* m, float* v, void* arena, int dtype, void* stream) {
  if (ngroups < 1 || ngroups > KLAB_ADAMW_MAX_GROUPS) return KLAB_ERR_UNSUPPORTED;
  if (!desc_dev || ndesc <= 0 || !group_of_dev || !groups || !grads || !m || !v || !arena || begin4 < 0 || end4 < begin4) return KLAB_ERR_BADARG;
  if (dtype != KLAB_BF16 && dtype != KLAB_F32) return KLAB_ERR_BADARG;
  AdamWGroups hy{};
  for (int i = 0; i < ngroups; ++i) {
    const klab_adamw_group& s = groups[i];
    if (!(s.bias_corr1 > 0.f) || !(s.bias_corr2 > 0.f)) return KLAB_ERR_BADARG;
    AdamWHyper& h = hy.g[i];
    h.decay = (float)(1.0 - (double)s.lr * (double)s.weight_decay);
    h.step = (float)((double)s.lr / (double)s.bias_corr1);
    h.one_minus_beta1 = 1.f - s.beta1; h.beta2 = s.beta2; h.one_minus_beta2 = 1.f - s.beta2;
    h.inv_sqrt_bc2 = 1.f / sqrtf(s.bias_corr2); h.eps = s.eps;
  }
  if (end4 == begin4) return KLAB_OK;
  mt_dispatch(dtype, arena, [&](auto* a) {
    hipLaunchKernelGGL((adamw_step_kernel<std::remove_pointer_t<decltype(a)>, MT_U>), dim3(mt_grid(end4 - begin4)), dim3(256), 0, (hipStream_t)stream,
                       (const AdamDesc*)desc_dev, ndesc, group_of_dev, begin4, end4, grads, m, v, a, hy);
  });
  KLAB_LAUNCH_CHECK();
  return KLAB_OK;
}
