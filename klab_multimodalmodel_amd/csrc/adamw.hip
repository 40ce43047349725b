// Fused multi-tensor AdamW (decoupled weight decay; torch.optim.AdamW's single-tensor rule without amsgrad / maximize) with
// per-GROUP hyper-parameters and the compute-dtype shadow copy the Adam step also writes (misc.hip, adam_step_kernel).
//
// One pass over the trainable tensors, whatever the number of parameter groups: p, g, m, v in as 16-byte non-temporal vectors,
// p, m, v out, and -- for tensors with aoff >= 0 -- the bf16 / f32 copy the next forward's GEMMs read, straight into the weight
// arena.  30 bytes per parameter, as Adam.
//
// Tables.  The engine's AdamDesc table {p, goff, aoff, n4_prefix} is used as it is.  A second device table, group_of[nd] in the
// same order, names each tensor's parameter group.  Both go to LDS when nd <= 1024 (the chain of dependent loads described at
// adam_step_kernel) and are read from global memory above that.  The groups' hyper-parameters (at most KLAB_ADAMW_MAX_GROUPS)
// arrive BY VALUE in the kernel arguments, already derived on the host, and are copied to LDS once per workgroup: no host ->
// device copy per step, no device -> host read, and no global load in front of the streaming loads that depends on another.
//
// Per element, in f32 and in this order (torch's order):
//   p'  = p * decay                               decay = (float)(1.0 - (double)lr * (double)weight_decay)
//   m'  = m + (1 - beta1) (g - m)
//   v'  = beta2 v + (1 - beta2) g^2
//   p'' = p' - step * (m' / (sqrt(v') * inv_sqrt_bc2 + eps))      step = (float)((double)lr / bias_corr1)
// lr = 0 gives decay = 1 and step = 0: p keeps its bits while m and v move on.
#include <math.h>

#include "common.h"
#include "klab_mm.h"

namespace klab {
namespace {

struct AdamDesc { float* p; long goff; long aoff; long n4_prefix; };  // the engine's table (misc.hip); aoff < 0: no arena copy
struct alignas(32) AdamWHyper { float decay, one_minus_beta1, beta2, one_minus_beta2, step, inv_sqrt_bc2, eps, pad; };
struct AdamWGroups { AdamWHyper g[KLAB_ADAMW_MAX_GROUPS]; };

static_assert((KLAB_ADAMW_MAX_GROUPS & (KLAB_ADAMW_MAX_GROUPS - 1)) == 0, "a group id is masked into the LDS table");

template <typename T, int U>
__global__ __launch_bounds__(256) void adamw_step_kernel(const AdamDesc* __restrict__ dglob, int nd, const int* __restrict__ group_of,
                                                         long begin4, long total4, const float* __restrict__ grads, float* __restrict__ m,
                                                         float* __restrict__ v, T* __restrict__ arena, const AdamWGroups hy) {
  constexpr int MAXD = 1024;  // (T5-large: ~560 tensors; 32 KiB + 1 KiB of group ids)
  __shared__ AdamDesc dsh[MAXD];
  __shared__ unsigned char gsh[MAXD];
  __shared__ AdamWHyper hsh[KLAB_ADAMW_MAX_GROUPS];
  const bool in_lds = nd <= MAXD;
  {
    constexpr int NW = (int)(sizeof(AdamWGroups) / sizeof(float));
    const float* src = reinterpret_cast<const float*>(&hy);
    float* dst = reinterpret_cast<float*>(hsh);
    for (int i = threadIdx.x; i < NW; i += blockDim.x) dst[i] = src[i];
  }
  if (in_lds)
    for (int i = threadIdx.x; i < nd; i += blockDim.x) { dsh[i] = dglob[i]; gsh[i] = (unsigned char)group_of[i]; }
  __syncthreads();
  const AdamDesc* d = in_lds ? dsh : dglob;
  // vec4 indices [begin4, total4) of the descriptor table's prefix space (a sub-range = the tensors of one backward segment)
  for (long g0 = begin4 + ((long)blockIdx.x * U) * blockDim.x + threadIdx.x; g0 < total4; g0 += (long)gridDim.x * U * blockDim.x) {
    int lo = 0, hi = nd - 1;
    while (lo < hi) {  // ONE search per thread and iteration, then a walk forward
      const int mid = (lo + hi + 1) >> 1;
      if (d[mid].n4_prefix <= g0) lo = mid; else hi = mid - 1;
    }
    f32x4 pv[U], gv[U], mv[U], vv[U];
    float* pp[U]; long go[U]; long ao[U]; int gi[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long g = g0 + (long)u * blockDim.x;
      pp[u] = nullptr;
      if (g < total4) {
        while (lo + 1 < nd && d[lo + 1].n4_prefix <= g) ++lo;
        const long local = (g - d[lo].n4_prefix) * 4;
        pp[u] = d[lo].p + local; go[u] = d[lo].goff + local; ao[u] = d[lo].aoff < 0 ? -1 : d[lo].aoff + local;
        // the group id is consumed only after the streaming loads below are in flight
        gi[u] = (in_lds ? (int)gsh[lo] : group_of[lo]) & (KLAB_ADAMW_MAX_GROUPS - 1);
        pv[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(pp[u]));
        gv[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(grads + go[u]));
        mv[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(m + go[u]));
        vv[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(v + go[u]));
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
        __builtin_nontemporal_store(po, reinterpret_cast<f32x4*>(pp[u]));
        __builtin_nontemporal_store(mo, reinterpret_cast<f32x4*>(m + go[u]));
        __builtin_nontemporal_store(vo, reinterpret_cast<f32x4*>(v + go[u]));
        if (ao[u] >= 0) {
          if constexpr (sizeof(T) == 2) *reinterpret_cast<bf16x4*>(arena + ao[u]) = bf16x4{(bf16_t)po[0], (bf16_t)po[1], (bf16_t)po[2], (bf16_t)po[3]};
          else *reinterpret_cast<f32x4*>(arena + ao[u]) = po;
        }
      }
  }
}

}  // namespace
}  // namespace klab

using namespace klab;

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
  hipStream_t s = (hipStream_t)stream;
  constexpr int ADAMW_GRID = 1024;  // the Adam step's launch shape (misc.hip): 4 workgroups per CU, 4 vec4 of each stream in flight per thread
  constexpr int U = 4;
  long gl = ((end4 - begin4 + U - 1) / U + 255) / 256;
  const unsigned grid = (unsigned)(gl < 1 ? 1 : (gl > ADAMW_GRID ? ADAMW_GRID : gl));
  if (dtype == KLAB_BF16)
    hipLaunchKernelGGL((adamw_step_kernel<bf16_t, U>), dim3(grid), dim3(256), 0, s, (const AdamDesc*)desc_dev, ndesc, group_of_dev, begin4, end4,
                       grads, m, v, (bf16_t*)arena, hy);
  else
    hipLaunchKernelGGL((adamw_step_kernel<float, U>), dim3(grid), dim3(256), 0, s, (const AdamDesc*)desc_dev, ndesc, group_of_dev, begin4, end4,
                       grads, m, v, (float*)arena, hy);
  KLAB_LAUNCH_CHECK();
  return KLAB_OK;
}
