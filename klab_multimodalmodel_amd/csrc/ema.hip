// Fused multi-tensor weight EMA over the engine's AdamDesc table {p, goff, aoff, n4_prefix} (misc.hip, adamw.hip), written the
// way adamw.hip is: one launch whatever the number of tensors, the table in LDS when nd <= 1024 and read from global memory above
// that, ONE binary search per thread and iteration and then a walk forward, 16-byte non-temporal loads and stores.
//
// Update.  ema is laid out like the "main" flat gradient buffer (indexed by goff, exactly as Adam's m and v).  Per element, in f32:
//   e' = e + w (p - e)                            w = (float)(1.0 - decay_t), a host scalar passed by value
// p is only read, no arena is touched: p, e in, e out -- 12 bytes per parameter.
//
// Swap.  p and e exchange their BITS (the vectors are moved, never computed with: NaN payloads, -0, infinities and denormals
// survive), and -- for tensors with aoff >= 0 -- the compute-dtype copy of the new p goes straight into the weight arena, the
// round-to-nearest-even bf16 cast or the f32 bits the optimizer steps write.  p, e in, p, e out: 16 bytes per parameter + 2 for
// the bf16 copy.  Two swaps restore p and e bit for bit.
#include "common.h"
#include "klab_mm.h"

namespace klab {
namespace {

struct AdamDesc { float* p; long goff; long aoff; long n4_prefix; };  // the engine's table (misc.hip); aoff < 0: no arena copy

constexpr int EMA_MAXD = 1024;  // (T5-large: ~560 tensors; 32 KiB)

// SWAP = false: e' = e + w (p - e).  SWAP = true: p <-> e and the arena copy of the new p (T = the arena's element type).
template <typename T, int U, bool SWAP>
__global__ __launch_bounds__(256) void ema_kernel(const AdamDesc* __restrict__ dglob, int nd, long begin4, long total4, float* __restrict__ ema,
                                                  float w, T* __restrict__ arena) {
  __shared__ AdamDesc dsh[EMA_MAXD];
  const bool in_lds = nd <= EMA_MAXD;
  if (in_lds)
    for (int i = threadIdx.x; i < nd; i += blockDim.x) dsh[i] = dglob[i];
  __syncthreads();
  const AdamDesc* d = in_lds ? dsh : dglob;
  // vec4 indices [begin4, total4) of the descriptor table's prefix space
  for (long g0 = begin4 + ((long)blockIdx.x * U) * blockDim.x + threadIdx.x; g0 < total4; g0 += (long)gridDim.x * U * blockDim.x) {
    int lo = 0, hi = nd - 1;
    while (lo < hi) {  // ONE search per thread and iteration, then a walk forward
      const int mid = (lo + hi + 1) >> 1;
      if (d[mid].n4_prefix <= g0) lo = mid; else hi = mid - 1;
    }
    f32x4 pv[U], ev[U];
    float* pp[U]; long go[U]; long ao[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long g = g0 + (long)u * blockDim.x;
      pp[u] = nullptr;
      if (g < total4) {
        while (lo + 1 < nd && d[lo + 1].n4_prefix <= g) ++lo;
        const long local = (g - d[lo].n4_prefix) * 4;
        pp[u] = d[lo].p + local; go[u] = d[lo].goff + local; ao[u] = d[lo].aoff < 0 ? -1 : d[lo].aoff + local;
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
          if (ao[u] >= 0) {
            const f32x4 po = ev[u];
            if constexpr (sizeof(T) == 2) *reinterpret_cast<bf16x4*>(arena + ao[u]) = bf16x4{(bf16_t)po[0], (bf16_t)po[1], (bf16_t)po[2], (bf16_t)po[3]};
            else *reinterpret_cast<f32x4*>(arena + ao[u]) = po;
          }
        } else {
          f32x4 eo;
#pragma unroll
          for (int i = 0; i < 4; ++i) eo[i] = ev[u][i] + w * (pv[u][i] - ev[u][i]);  // shadow.lerp_(param, w)
          __builtin_nontemporal_store(eo, reinterpret_cast<f32x4*>(ema + go[u]));
        }
      }
  }
}

constexpr int EMA_GRID = 1024;  // the Adam step's launch shape (misc.hip): 4 workgroups per CU, 4 vec4 of each stream in flight per thread
constexpr int EMA_U = 4;

unsigned ema_grid(long n4) {
  const long gl = ((n4 + EMA_U - 1) / EMA_U + 255) / 256;
  return (unsigned)(gl < 1 ? 1 : (gl > EMA_GRID ? EMA_GRID : gl));
}

}  // namespace
}  // namespace klab

using namespace klab;

extern "C" int klab_ema_update_range(const void* desc_dev, int ndesc, long begin4, long end4, float* ema, float w, void* stream) {
  if (!desc_dev || ndesc <= 0 || !ema || begin4 < 0 || end4 < begin4) return KLAB_ERR_BADARG;
  if (!(w >= 0.f && w <= 1.f)) return KLAB_ERR_BADARG;  // (NaN fails both comparisons)
  if (end4 == begin4) return KLAB_OK;
  hipLaunchKernelGGL((ema_kernel<float, EMA_U, false>), dim3(ema_grid(end4 - begin4)), dim3(256), 0, (hipStream_t)stream,
                     (const AdamDesc*)desc_dev, ndesc, begin4, end4, ema, w, (float*)nullptr);
  KLAB_LAUNCH_CHECK();
  return KLAB_OK;
}

extern "C" int klab_ema_swap_range(const void* desc_dev, int ndesc, long begin4, long end4, float* ema, void* arena, int dtype, void* stream) {
  if (!desc_dev || ndesc <= 0 || !ema || !arena || begin4 < 0 || end4 < begin4) return KLAB_ERR_BADARG;
  if (dtype != KLAB_BF16 && dtype != KLAB_F32) return KLAB_ERR_BADARG;
  if (end4 == begin4) return KLAB_OK;
  hipStream_t s = (hipStream_t)stream;
  const unsigned grid = ema_grid(end4 - begin4);
  if (dtype == KLAB_BF16)
    hipLaunchKernelGGL((ema_kernel<bf16_t, EMA_U, true>), dim3(grid), dim3(256), 0, s, (const AdamDesc*)desc_dev, ndesc, begin4, end4, ema, 0.f,
                       (bf16_t*)arena);
  else
    hipLaunchKernelGGL((ema_kernel<float, EMA_U, true>), dim3(grid), dim3(256), 0, s, (const AdamDesc*)desc_dev, ndesc, begin4, end4, ema, 0.f,
                       (float*)arena);
  KLAB_LAUNCH_CHECK();
  return KLAB_OK;
}
