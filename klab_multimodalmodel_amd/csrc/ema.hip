// Fused multi-tensor weight EMA over the engine's AdamDesc table, walked and launched as multi_tensor.h describes: one launch
// whatever the number of tensors, 16-byte non-temporal loads and stores.
//
// Update.  ema is laid out like the "main" flat gradient buffer (indexed by goff, exactly as Adam's m and v).  Per element, in f32:
//   e' = e + w (p - e)                            w = (float)(1.0 - decay_t), a host scalar passed by value
// p is only read, no arena is touched: p, e in, e out -- 12 bytes per parameter.
//
// Swap.  p and e exchange their BITS (the vectors are moved, never computed with: NaN payloads, -0, infinities and denormals
// survive), and -- for tensors with aoff >= 0 -- the compute-dtype copy of the new p goes straight into the weight arena, the
// round-to-nearest-even bf16 cast or the f32 bits the optimizer steps write.  p, e in, p, e out: 16 bytes per parameter + 2 for
// the bf16 copy.  Two swaps restore p and e bit for bit.
#include <type_traits>

#include "common.h"
#include "klab_mm.h"
#include "multi_tensor.h"

namespace klab {
namespace {

// SWAP = false: e' = e + w (p - e).  SWAP = true: p <-> e and the arena copy of the new p (T = the arena's element type).
template <typename T, int U, bool SWAP>
__global__ __launch_bounds__(256) void ema_kernel(const AdamDesc* __restrict__ dglob, int nd, long begin4, long total4, float* __restrict__ ema,
                                                  float w, T* __restrict__ arena) {
  __shared__ AdamDesc dsh[MT_MAXD];
  TableWalker<AdamDesc> tw{mt_stage_table(dsh, dglob, nd), nd, 0};
  // vec4 indices [begin4, total4) of the descriptor table's prefix space
  for (long g0 = begin4 + ((long)blockIdx.x * U) * blockDim.x + threadIdx.x; g0 < total4; g0 += (long)gridDim.x * U * blockDim.x) {
    tw.seek(g0);
    f32x4 pv[U], ev[U];
    float* pp[U]; long go[U]; long ao[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long g = g0 + (long)u * blockDim.x;
      pp[u] = nullptr;
      if (g < total4) {
        const long local = tw.advance(g);
        const AdamDesc& d = tw.cur();
        pp[u] = d.p + local; go[u] = d.goff + local; ao[u] = d.aoff < 0 ? -1 : d.aoff + local;
        pv[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(pp[u]));
        ev[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(ema + go[u]));
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (pp[u]) {
        if constexpr (SWAP) {
          __builtin_nontemporal_store(ev[u], reinterpret_cast<f32x4*>(pp[u]));
          __builtin_nontemporal_store(pv[u], reinterpret_cast<f32x4*>(ema + go[u]));
          if (ao[u] >= 0) mt_store_vec4(arena + ao[u], ev[u]);
        } else {
          f32x4 eo;
#pragma unroll
          for (int i = 0; i < 4; ++i) eo[i] = ev[u][i] + w * (pv[u][i] - ev[u][i]);  // shadow.lerp_(param, w)
          __builtin_nontemporal_store(eo, reinterpret_cast<f32x4*>(ema + go[u]));
        }
      }
  }
}

}  // namespace
}  // namespace klab

using namespace klab;

extern "C" int klab_ema_update_range(const void* desc_dev, int ndesc, long begin4, long end4, float* ema, float w, void* stream) {
  if (!desc_dev || ndesc <= 0 || !ema || begin4 < 0 || end4 < begin4) return KLAB_ERR_BADARG;
  if (!(w >= 0.f && w <= 1.f)) return KLAB_ERR_BADARG;  // (NaN fails both comparisons)
  if (end4 == begin4) return KLAB_OK;
  hipLaunchKernelGGL((ema_kernel<float, MT_U, false>), dim3(mt_grid(end4 - begin4)), dim3(256), 0, (hipStream_t)stream,
                     (const AdamDesc*)desc_dev, ndesc, begin4, end4, ema, w, (float*)nullptr);
  KLAB_LAUNCH_CHECK();
  return KLAB_OK;
}

extern "C" int klab_ema_swap_range(const void* desc_dev, int ndesc, long begin4, long end4, float* ema, void* arena, int dtype, void* stream) {
  if (!desc_dev || ndesc <= 0 || !ema || !arena || begin4 < 0 || end4 < begin4) return KLAB_ERR_BADARG;
  if (dtype != KLAB_BF16 && dtype != KLAB_F32) return KLAB_ERR_BADARG;
  if (end4 == begin4) return KLAB_OK;
  mt_dispatch(dtype, arena, [&](auto* a) {
    hipLaunchKernelGGL((ema_kernel<std::remove_pointer_t<decltype(a)>, MT_U, true>), dim3(mt_grid(end4 - begin4)), dim3(256), 0, (hipStream_t)stream,
                       (const AdamDesc*)desc_dev, ndesc, begin4, end4, ema, 0.f, a);
  });
  KLAB_LAUNCH_CHECK();
  return KLAB_OK;
}
