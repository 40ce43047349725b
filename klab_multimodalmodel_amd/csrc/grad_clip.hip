// Multi-tensor gradient norm and in-place gradient scale (torch.nn.utils.clip_grad_norm_ for fp32 gradients that live anywhere
// on one device: the engine's flat buffers and foreign tensors alike).  The table is a device array of {float* ptr; long n}, one
// entry per gradient tensor, n >= 1.
//
//   klab_grad_norm   launch 1  one fp64 partial per CHUNK of GC_CHUNK elements; tensor i owns ceil(n_i / GC_CHUNK) consecutive ones
//                    launch 2  one workgroup: per-tensor sums of the partials, then their sum, both in index order
//   klab_grad_clip   one launch: coef = clamp(max_norm / (total + 1e-6), max = 1); g *= coef, or nothing at all when coef >= 1
//
// Why fp64: the square of an fp32 value has at most 48 significant bits, so  (double)g * (double)g  is exact, and sums of such
// squares stay finite up to 2^1023 (torch's fp32 squares overflow above a norm of 1.8e19).  What remains is the rounding of the
// fp64 additions, about n * 2^-53 relative.
//
// Nothing in this file is a floating-point atomic, and every sum runs in an order that depends on the table alone (a thread's
// elements, the wave's lanes, the workgroup's waves, the tensor's partials, the tensors): the same input gives the same bits on
// every run and for every grid size.  Max-abs (kind 1, torch's norm_type = inf) goes through the same path with a maximum that
// keeps NaN (fmax would drop it).
//
// A workgroup finds the tensor that owns a chunk by a binary search over the prefix sums of the tensors' partial counts.  Those
// are built in LDS, from a tile of up to GC_MAXT table entries at a time: a table of up to 1024 tensors is read once per
// workgroup and the search never leaves LDS (the chain of dependent loads described in multi_tensor.h); a longer
// table is walked tile by tile from global memory.
#include <math.h>

#include "common.h"
#include "klab_mm.h"

namespace klab {

struct GcEntry { float* ptr; long n; };

constexpr int GC_CHUNK = 32768;  // elements per partial: 128 KiB, 32 vec4 per thread of a 256-thread workgroup
constexpr int GC_MAXT = 1024;    // table entries per LDS tile (T5-large: ~560 tensors)
constexpr int GC_GRID = 2048;    // 256 CUs x 8 workgroups
constexpr int GC_SMALL = 32;     // launch 2: tensors of up to this many partials are summed by one thread each, longer ones by a wave
enum { GC_L2 = 0, GC_MAXABS = 1 };

static_assert(GC_CHUNK % 1024 == 0, "a chunk is whole vec4 rounds of the workgroup and keeps the tensor's 16-byte alignment");

// the reduction's one operation.  L2: a sum.  Max-abs: a maximum in which NaN, once seen, stays: a NaN operand is taken by its
// own test, and nothing compares greater than a NaN accumulator
template <int KIND> __device__ __forceinline__ double gc_comb(double acc, double x) {
  if constexpr (KIND == GC_L2) return acc + x;
  else return (x > acc || x != x) ? x : acc;
}
template <int KIND> __device__ __forceinline__ double gc_elem(float g) {
  const double d = (double)g;
  if constexpr (KIND == GC_L2) return d * d;  // exact
  else return fabs(d);
}
template <int KIND> __device__ __forceinline__ float gc_final(double s) {
  if constexpr (KIND == GC_L2) return (float)sqrt(s);
  else return (float)s;
}

__device__ __forceinline__ long gc_count(long n) { return n > 0 ? (n + GC_CHUNK - 1) / GC_CHUNK : 0; }

// Exclusive prefix sums of the partial counts of table entries [base, base + cnt), cnt <= GC_MAXT, into pre[0 .. cnt]
// (pre[cnt] = the tile's total).  BLOCK threads, GC_MAXT / BLOCK consecutive entries per thread.  Ends with a barrier.
template <int BLOCK>
__device__ __forceinline__ void gc_scan_tile(const GcEntry* __restrict__ tab, int base, int cnt, GcEntry* esh, long* pre, long* wtot) {
  constexpr int ITEMS = GC_MAXT / BLOCK, NW = BLOCK / 64;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  long c[ITEMS], mine = 0;
#pragma unroll
  for (int j = 0; j < ITEMS; ++j) {
    const int i = t * ITEMS + j;
    c[j] = 0;
    if (i < cnt) {
      const GcEntry e = tab[base + i];
      if (esh) esh[i] = e;
      c[j] = gc_count(e.n);
    }
    mine += c[j];
  }
  long incl = mine;  // inclusive scan over the wave's lanes
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const long up = __shfl_up(incl, o, 64);
    if (lane >= o) incl += up;
  }
  if (lane == 63) wtot[w] = incl;
  __syncthreads();
  long off = incl - mine;
  for (int k = 0; k < w; ++k) off += wtot[k];
#pragma unroll
  for (int j = 0; j < ITEMS; ++j) {
    const int i = t * ITEMS + j;
    if (i < cnt) pre[i] = off;
    off += c[j];
  }
  if (t == BLOCK - 1) pre[cnt] = off;  // the last thread's running sum is the tile's total (entries past cnt count 0)
  __syncthreads();
}

// last i in [0, cnt) with pre[i] <= c, for 0 <= c < pre[cnt]
__device__ __forceinline__ int gc_find(const long* pre, int cnt, long c) {
  int lo = 0, hi = cnt - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (pre[mid] <= c) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// Calls f(entry, chunk index inside the tensor, global chunk index) for every chunk this workgroup owns under a grid stride,
// with all 256 threads.  `limit` bounds the global chunk index (the caller's partial buffer).
template <typename F>
__device__ __forceinline__ void gc_for_each_chunk(const GcEntry* __restrict__ tab, int nt, long limit, F f) {
  __shared__ GcEntry esh[GC_MAXT];
  __shared__ long pre[GC_MAXT + 1];
  __shared__ long wtot[4];
  long run = 0, c = blockIdx.x;
  for (int base = 0; base < nt; base += GC_MAXT) {
    const int cnt = nt - base < GC_MAXT ? nt - base : GC_MAXT;
    if (base) __syncthreads();  // the previous tile's esh / pre are still being read
    gc_scan_tile<256>(tab, base, cnt, esh, pre, wtot);
    const long end = run + pre[cnt] < limit ? run + pre[cnt] : limit;
    for (; c < end; c += gridDim.x) {
      const int i = gc_find(pre, cnt, c - run);
      f(esh[i], c - run - pre[i], c);
    }
    run += pre[cnt];
  }
}

// ---- launch 1: one partial per chunk --------------------------------------------------------------------------------------------
// A thread folds its own elements in the order it meets them (vec4 t, t + 256, ... of the chunk, or elements t, t + 256, ... when
// the tensor is not 16-byte aligned), the wave folds its lanes by an xor butterfly, thread 0 folds the four waves in order.
// The pointers come out of the table, so the compiler cannot see that they are global memory: say so (global_load / global_store
// instead of flat ones).  Whole rounds of U accesses per thread run without a bounds test -- U loads in flight; a select per
// load makes hipcc wait for each one -- and what is left goes one access at a time.  The order of a thread's elements is the
// same either way.
typedef __attribute__((address_space(1))) float gfloat;
typedef __attribute__((address_space(1))) f32x4 gf32x4;
constexpr int GC_U = 8;

template <int KIND> __device__ __forceinline__ double gc_fold(double acc, float x) { return gc_comb<KIND>(acc, gc_elem<KIND>(x)); }
template <int KIND> __device__ __forceinline__ double gc_fold(double acc, f32x4 x) {
#pragma unroll
  for (int i = 0; i < 4; ++i) acc = gc_comb<KIND>(acc, gc_elem<KIND>(x[i]));
  return acc;
}

template <int KIND, typename T>  // n items of T (f32x4 or float) at p
__device__ __forceinline__ double gc_stream_fold(double acc, const __attribute__((address_space(1))) T* p, int n) {
  int v0 = threadIdx.x;
  for (; v0 + (GC_U - 1) * 256 < n; v0 += 256 * GC_U) {
    T x[GC_U];
#pragma unroll
    for (int u = 0; u < GC_U; ++u) x[u] = p[v0 + u * 256];
#pragma unroll
    for (int u = 0; u < GC_U; ++u) acc = gc_fold<KIND>(acc, x[u]);
  }
  for (; v0 < n; v0 += 256) acc = gc_fold<KIND>(acc, p[v0]);
  return acc;
}

template <typename T>
__device__ __forceinline__ void gc_stream_scale(__attribute__((address_space(1))) T* p, int n, float coef) {
  int v0 = threadIdx.x;
  for (; v0 + (GC_U - 1) * 256 < n; v0 += 256 * GC_U) {
    T x[GC_U];
#pragma unroll
    for (int u = 0; u < GC_U; ++u) x[u] = p[v0 + u * 256];
#pragma unroll
    for (int u = 0; u < GC_U; ++u) p[v0 + u * 256] = x[u] * coef;
  }
  for (; v0 < n; v0 += 256) p[v0] = p[v0] * coef;
}

template <int KIND>
__device__ __forceinline__ double gc_chunk_reduce(const float* p, int len, double* red) {
  double acc = 0.0;
  const int t = threadIdx.x;
  if ((reinterpret_cast<uintptr_t>(p) & 15) == 0) {
    const int nv = len >> 2;
    acc = gc_stream_fold<KIND, f32x4>(acc, (const gf32x4*)p, nv);
    const int e = (nv << 2) + t;  // the tensor's last 1 - 3 elements
    if (e < len) acc = gc_fold<KIND>(acc, ((const gfloat*)p)[e]);
  } else {
    acc = gc_stream_fold<KIND, float>(acc, (const gfloat*)p, len);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc = gc_comb<KIND>(acc, __shfl_xor(acc, o, 64));
  __syncthreads();  // red may still be read from the previous chunk
  if ((t & 63) == 0) red[t >> 6] = acc;
  __syncthreads();
  return gc_comb<KIND>(gc_comb<KIND>(gc_comb<KIND>(red[0], red[1]), red[2]), red[3]);
}

template <int KIND>
__global__ __launch_bounds__(256) void grad_norm_partial_kernel(const GcEntry* __restrict__ tab, int nt, double* __restrict__ parts, long nparts) {
  __shared__ double red[4];
  gc_for_each_chunk(tab, nt, nparts, [&](const GcEntry& e, long k, long c) {
    const long e0 = k * GC_CHUNK;
    const int len = (int)(e.n - e0 < GC_CHUNK ? e.n - e0 : GC_CHUNK);
    const double s = gc_chunk_reduce<KIND>(e.ptr + e0, len, red);
    if (threadIdx.x == 0) parts[c] = s;
  });
}

// ---- launch 2: per-tensor results and the total ------------------------------------------------------------------------------------
// acc folded with the 64 lanes' values in lane order, the same in every lane
template <int KIND> __device__ __forceinline__ double gc_wave_ordered(double acc, double v) {
  for (int l = 0; l < 64; ++l) acc = gc_comb<KIND>(acc, __shfl(v, l, 64));
  return acc;
}

template <int KIND>
__global__ __launch_bounds__(1024) void grad_norm_final_kernel(const GcEntry* __restrict__ tab, int nt, const double* __restrict__ parts, long nparts,
                                                               float* __restrict__ norms) {
  __shared__ long pre[GC_MAXT + 1];
  __shared__ long wtot[16];
  __shared__ double ssh[GC_MAXT];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  long run = 0;
  double total = 0.0;  // wave 0's, identical in its lanes
  for (int base = 0; base < nt; base += GC_MAXT) {
    const int cnt = nt - base < GC_MAXT ? nt - base : GC_MAXT;
    if (base) __syncthreads();
    gc_scan_tile<1024>(tab, base, cnt, nullptr, pre, wtot);
    // Both forms add a tensor's partials strictly in index order, so which one a tensor takes changes no bit.  A partial
    // that the caller's buffer does not hold reads as NaN.
    if (t < cnt) {
      const long first = run + pre[t], np = pre[t + 1] - pre[t];
      if (np <= GC_SMALL) {
        double s = 0.0;
        for (long k = 0; k < np; k += 8) {
          double x[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) x[j] = k + j < np ? (first + k + j < nparts ? parts[first + k + j] : (double)NAN) : 0.0;
#pragma unroll
          for (int j = 0; j < 8; ++j) s = gc_comb<KIND>(s, x[j]);  // 0 is the identity of both kinds
        }
        ssh[t] = s;
        norms[base + t] = gc_final<KIND>(s);
      }
    }
    for (int i = w; i < cnt; i += 16) {
      const long first = run + pre[i], np = pre[i + 1] - pre[i];
      if (np <= GC_SMALL) continue;
      double s = 0.0;
      for (long k = 0; k < np; k += 64) {
        const long idx = first + k + lane;
        const double x = k + lane < np ? (idx < nparts ? parts[idx] : (double)NAN) : 0.0;
        s = gc_wave_ordered<KIND>(s, x);
      }
      if (lane == 0) {
        ssh[i] = s;
        norms[base + i] = gc_final<KIND>(s);
      }
    }
    __syncthreads();
    if (w == 0)
      for (int k = 0; k < cnt; k += 64) total = gc_wave_ordered<KIND>(total, k + lane < cnt ? ssh[k + lane] : 0.0);
    run += pre[cnt];
  }
  if (t == 0) norms[nt] = gc_final<KIND>(total);
}

// ---- clip ----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void grad_clip_kernel(const GcEntry* __restrict__ tab, int nt, const float* __restrict__ total_dev, float max_norm,
                                                        float* __restrict__ coef_dev) {
  const float c = max_norm / (*total_dev + 1e-6f);
  const float coef = c < 1.f ? c : (c >= 1.f ? 1.f : c);  // torch's clamp(max = 1): NaN stays
  if (blockIdx.x == 0 && threadIdx.x == 0) coef_dev[0] = coef;
  if (coef >= 1.f) return;  // uniform over the grid: nothing is clipped, nothing is read or written
  gc_for_each_chunk(tab, nt, 0x7fffffffffffffffL, [&](const GcEntry& e, long k, long) {
    const long e0 = k * GC_CHUNK;
    const int len = (int)(e.n - e0 < GC_CHUNK ? e.n - e0 : GC_CHUNK);
    float* p = e.ptr + e0;
    if ((reinterpret_cast<uintptr_t>(p) & 15) == 0) {
      const int nv = len >> 2;
      gc_stream_scale<f32x4>((gf32x4*)p, nv, coef);
      const int el = (nv << 2) + (int)threadIdx.x;  // the tensor's last 1 - 3 elements
      if (el < len) ((gfloat*)p)[el] *= coef;
    } else {
      gc_stream_scale<float>((gfloat*)p, len, coef);
    }
  });
}

}  // namespace klab

using namespace klab;

extern "C" int klab_grad_norm_chunk(void) { return GC_CHUNK; }

extern "C" int klab_grad_norm(const void* table_dev, int nt, int kind, double* parts, long nparts, float* norms, void* stream) {
  // every tensor owns at least one partial; the exact count is known to the device only, where launch 1 never writes past
  // nparts and launch 2 turns a missing partial into NaN
  if (nt < 0 || (nt > 0 && (!table_dev || !parts)) || !norms || nparts < nt || (kind != GC_L2 && kind != GC_MAXABS)) return KLAB_ERR_BADARG;
  const GcEntry* tab = (const GcEntry*)table_dev;
  hipStream_t s = (hipStream_t)stream;
  if (nt > 0) {
    const unsigned grid = (unsigned)(nparts < GC_GRID ? nparts : GC_GRID);
    if (kind == GC_L2) hipLaunchKernelGGL(grad_norm_partial_kernel<GC_L2>, dim3(grid), dim3(256), 0, s, tab, nt, parts, nparts);
    else hipLaunchKernelGGL(grad_norm_partial_kernel<GC_MAXABS>, dim3(grid), dim3(256), 0, s, tab, nt, parts, nparts);
  }
  if (kind == GC_L2) hipLaunchKernelGGL(grad_norm_final_kernel<GC_L2>, dim3(1), dim3(1024), 0, s, tab, nt, (const double*)parts, nparts, norms);
  else hipLaunchKernelGGL(grad_norm_final_kernel<GC_MAXABS>, dim3(1), dim3(1024), 0, s, tab, nt, (const double*)parts, nparts, norms);
  KLAB_LAUNCH_CHECK();
  return KLAB_OK;
}

extern "C" int klab_grad_clip(const void* table_dev, int nt, const float* total_dev, float max_norm, float* coef_dev, void* stream) {
  if (nt < 0 || (nt > 0 && !table_dev) || !total_dev || !coef_dev || total_dev == coef_dev) return KLAB_ERR_BADARG;
  // the sizes are in the device table: a fixed grid strides over the chunks it finds there
  hipLaunchKernelGGL(grad_clip_kernel, dim3(nt > 0 ? GC_GRID : 1), dim3(256), 0, (hipStream_t)stream, (const GcEntry*)table_dev, nt, total_dev, max_norm,
                     coef_dev);
  KLAB_LAUNCH_CHECK();
  return KLAB_OK;
}
