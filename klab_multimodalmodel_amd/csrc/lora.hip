// LoRA adapters in merged-weight form over a LoraDesc table (multi_tensor.h): one launch whatever the number of tensors.
//
//   klab_lora_merge   arena[aoff + i*in + j] = cast(W[i,j] + s * sum_k B[i,k] A[k,j])      (or the same f32 value into W itself)
//   klab_lora_grads   dB[i,k] = s * sum_j dW[i,j] A[k,j]       dA[k,j] = s * sum_i B[i,k] dW[i,j]       from dW in the flat buffer
//
// A workgroup's unit is a ROW BLOCK: LR_ROWS rows of one tensor, all columns, swept in tiles of LR_COLS columns.  Units are
// numbered through the table's rb_prefix; a fixed grid strides over them and finds a unit's descriptor by a binary search in
// the LDS copy of the table (mt_stage_table; dynamic LDS: nd descriptors, then the tiles).
//
// Arithmetic.  f32 FMAs only (no bf16 operand anywhere, no MFMA): the rank-r product is a k-ordered FMA chain per element.  The
// rank is padded with zeros in LDS to RP = 8, 16, 32 or 64 (exact: a zero product changes no sum), and the body is compiled
// for each RP; the descriptor's r picks it, so one table may mix ranks.
//   merge   acc = fma chain over k (r roundings), v = fma(s, acc, W) (one more); one rounding into the arena type.
//           B = 0 gives acc = +0 and v = W bit for bit (a master that is -0 becomes +0).
//   grads   launch 1 reads every dW element ONCE into an LDS tile.  From it the workgroup finishes its rows of dB (an FMA chain over
//           all columns in ascending order, times s) and stores its partial of dA (an FMA chain over its rows in ascending order,
//           unscaled) into the caller's slab [blocks, r, in] of the tensor.  Launch 2 adds a tensor's partials in block order and
//           scales by s.  No floating-point atomic, every order fixed by the table alone: the same bits on every run.
//           Both outputs are stored, never added to; dW, A and B are only read.
//
// Thread maps (256 threads, t = threadIdx.x), chosen so that every LDS read is a 16-byte read without bank conflicts:
//   merge   t & 15 = vec4 column of the tile, t >> 4 = group of 4 rows: 16 accumulators, W straight from global into registers
//           (issued before the tile of A is staged), per 4 ranks 4 reads of A and 4 of B for 64 FMAs.
//   dA      t & 15 = vec4 column, t >> 4 = group of RP / 16 ranks (RP = 8: half the threads), a chain over the 64 rows.
//   dB      t >> 3 = pair of rows, t & 7 = ranks t & 7, + 8, ... (RP / 8 of them), a chain over the tile's columns.
// Tried and not kept: loading the NEXT tile of dW and of A into registers before computing on the current one changed the gradient
// kernel's time by under 1 % at r = 8 and made it 5 - 10 % slower at r = 64 (T5-large: 8.28 against 7.54 ms): the kernel waits on
// its LDS reads, not on HBM -- at r = 8 the dA map uses a 16-byte LDS read for 4 FMAs.
// The merge moves 4 B in and 2 B out per element, and the tile of A (r * 256 B per 64 x 64 tile, from L2) beside it.  W and dW are
// touched once: non-temporal loads.  The arena is read by the forward right behind the merge: plain stores.
#include <type_traits>

#include "common.h"
#include "klab_mm.h"
#include "multi_tensor.h"

namespace klab {
namespace {

constexpr int LR_ROWS = 64;            // rows per unit
constexpr int LR_COLS = 64;            // columns per tile
constexpr int LR_LD = LR_COLS + 4;     // LDS row stride of a column tile (floats): rows 16 bytes apart in the banks
constexpr int LR_RMAX = 64;            // largest rank
constexpr int LR_GRID = 1024;          // 4 workgroups per CU, grid-stride over the units
constexpr int LR_BS = LR_ROWS * (LR_RMAX + 4);  // floats of the B tile [LR_ROWS][RP + 4]
constexpr int LR_TILE = LR_RMAX * LR_LD;        // floats of the A tile [RP][LR_LD] and of the dW tile [LR_ROWS][LR_LD]
static_assert(LR_ROWS == LR_RMAX, "the dW tile and the A tile share LR_TILE");

inline size_t lr_table_bytes(int nd) { return ((size_t)nd * sizeof(LoraDesc) + 15) & ~(size_t)15; }

__device__ __forceinline__ long lr_blocks(const LoraDesc& d) { return (d.out + LR_ROWS - 1) / LR_ROWS; }

// last i with rb_prefix[i] <= u, for 0 <= u < total units
__device__ __forceinline__ int lr_find(const LoraDesc* d, int nd, long u) {
  int lo = 0, hi = nd - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (d[mid].rb_prefix <= u) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// rows [row0, row0 + LR_ROWS) of B [out, r] -> Bs [LR_ROWS][RP + 4], zeros beyond out and r
template <int RP>
__device__ __forceinline__ void lr_stage_b(const LoraDesc& d, long row0, float* Bs) {
  for (int idx = threadIdx.x; idx < LR_ROWS * RP; idx += 256) {
    const int i = idx / RP, k = idx % RP;
    Bs[i * (RP + 4) + k] = (row0 + i < d.out && k < d.r) ? d.b[(row0 + i) * d.r + k] : 0.f;
  }
}

// columns [col0, col0 + LR_COLS) of A [r, in] -> As [RP][LR_LD], zeros beyond r and in
template <int RP>
__device__ __forceinline__ void lr_stage_a(const LoraDesc& d, int col0, float* As) {
  for (int idx = threadIdx.x; idx < RP * (LR_COLS / 4); idx += 256) {
    const int k = idx / (LR_COLS / 4), c4 = idx % (LR_COLS / 4);
    const int j = col0 + c4 * 4;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (k < d.r && j < d.in) v = *reinterpret_cast<const f32x4*>(d.a + (long)k * d.in + j);
    *reinterpret_cast<f32x4*>(As + k * LR_LD + c4 * 4) = v;
  }
}

// ---- merge ------------------------------------------------------------------------------------------------------------------------
template <typename T, int RP, bool TO_MASTER>
__device__ __forceinline__ void lr_merge_unit(const LoraDesc& d, long row0, T* __restrict__ arena, float* Bs, float* As) {
  constexpr int LB = RP + 4;
  const int cg = threadIdx.x & 15, rg = threadIdx.x >> 4;
  const float s = d.s;
  for (int col0 = 0; col0 < d.in; col0 += LR_COLS) {
    const int j = col0 + cg * 4;
    f32x4 w[4];
    bool ok[4];
#pragma unroll
    for (int ii = 0; ii < 4; ++ii) {
      const long i = row0 + rg * 4 + ii;
      ok[ii] = i < d.out && j < d.in;
      if (ok[ii]) w[ii] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(d.w + i * d.in + j));
    }
    __syncthreads();  // the previous tile's (and unit's) LDS reads are done
    if (col0 == 0) lr_stage_b<RP>(d, row0, Bs);
    lr_stage_a<RP>(d, col0, As);
    __syncthreads();
    f32x4 acc[4];
#pragma unroll
    for (int ii = 0; ii < 4; ++ii) acc[ii] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
    for (int k0 = 0; k0 < RP; k0 += 4) {
      f32x4 a[4];
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) a[kk] = *reinterpret_cast<const f32x4*>(As + (k0 + kk) * LR_LD + cg * 4);
#pragma unroll
      for (int ii = 0; ii < 4; ++ii) {
        const f32x4 b = *reinterpret_cast<const f32x4*>(Bs + (rg * 4 + ii) * LB + k0);
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) acc[ii] = b[kk] * a[kk] + acc[ii];
      }
    }
#pragma unroll
    for (int ii = 0; ii < 4; ++ii)
      if (ok[ii]) {
        const long e = (row0 + rg * 4 + ii) * d.in + j;
        const f32x4 v = s * acc[ii] + w[ii];
        if constexpr (TO_MASTER) *reinterpret_cast<f32x4*>(d.w + e) = v;
        else mt_store_vec4(arena + d.aoff + e, v);
      }
  }
}

template <typename T, bool TO_MASTER>
__global__ __launch_bounds__(256) void lora_merge_kernel(const LoraDesc* __restrict__ dglob, int nd, T* __restrict__ arena) {
  extern __shared__ __attribute__((aligned(16))) char lr_smem[];
  LoraDesc* dsh = reinterpret_cast<LoraDesc*>(lr_smem);
  float* Bs = reinterpret_cast<float*>(lr_smem + (((size_t)nd * sizeof(LoraDesc) + 15) & ~(size_t)15));
  float* As = Bs + LR_BS;
  const LoraDesc* tab = mt_stage_table(dsh, dglob, nd);
  const long total = tab[nd - 1].rb_prefix + lr_blocks(tab[nd - 1]);
  for (long u = blockIdx.x; u < total; u += gridDim.x) {
    const LoraDesc& d = tab[lr_find(tab, nd, u)];
    const long row0 = (u - d.rb_prefix) * LR_ROWS;
    if (d.r <= 8) lr_merge_unit<T, 8, TO_MASTER>(d, row0, arena, Bs, As);
    else if (d.r <= 16) lr_merge_unit<T, 16, TO_MASTER>(d, row0, arena, Bs, As);
    else if (d.r <= 32) lr_merge_unit<T, 32, TO_MASTER>(d, row0, arena, Bs, As);
    else lr_merge_unit<T, 64, TO_MASTER>(d, row0, arena, Bs, As);
  }
}

// ---- gradients, launch 1 -------------------------------------------------------------------------------------------------------------
template <int RP>
__device__ __forceinline__ void lr_grads_unit(const LoraDesc& d, long blk, const float* __restrict__ grads, float* __restrict__ out,
                                              float* __restrict__ slab, float* Bs, float* As, float* Ds) {
  constexpr int LB = RP + 4;
  constexpr int KA = RP >= 16 ? RP / 16 : 1;  // ranks per thread of the dA map
  constexpr int KG = RP / 8;                  // ranks per thread of the dB map
  const int t = threadIdx.x;
  const int cgA = t & 15, kA0 = (t >> 4) * KA;
  const int rB = (t >> 3) * 2, kB0 = t & 7;
  const long row0 = blk * LR_ROWS;
  const float* dw = grads + d.goff;
  float* part = slab + d.slab_off + blk * d.r * (long)d.in;
  float accB[2][KG];
#pragma unroll
  for (int kk = 0; kk < KG; ++kk) accB[0][kk] = accB[1][kk] = 0.f;
  for (int col0 = 0; col0 < d.in; col0 += LR_COLS) {
    f32x4 g[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long i = row0 + (t >> 4) + 16 * u;
      const int j = col0 + cgA * 4;
      g[u] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (i < d.out && j < d.in) g[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(dw + i * d.in + j));
    }
    __syncthreads();  // the previous tile's (and unit's) LDS reads are done
    if (col0 == 0) lr_stage_b<RP>(d, row0, Bs);
    lr_stage_a<RP>(d, col0, As);
#pragma unroll
    for (int u = 0; u < 4; ++u) *reinterpret_cast<f32x4*>(Ds + ((t >> 4) + 16 * u) * LR_LD + cgA * 4) = g[u];
    __syncthreads();
    if (kA0 < RP) {  // dA partial of this tile's columns: a chain over the unit's rows
      f32x4 acc[KA];
#pragma unroll
      for (int kk = 0; kk < KA; ++kk) acc[kk] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
      for (int i = 0; i < LR_ROWS; ++i) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(Ds + i * LR_LD + cgA * 4);
#pragma unroll
        for (int kk = 0; kk < KA; ++kk) acc[kk] = Bs[i * LB + kA0 + kk] * x + acc[kk];
      }
      const int j = col0 + cgA * 4;
#pragma unroll
      for (int kk = 0; kk < KA; ++kk)
        if (kA0 + kk < d.r && j < d.in) *reinterpret_cast<f32x4*>(part + (long)(kA0 + kk) * d.in + j) = acc[kk];
    }
#pragma unroll 2
    for (int c4 = 0; c4 < LR_COLS / 4; ++c4) {  // dB of the unit's rows: the chain goes on over this tile's columns
      const f32x4 x0 = *reinterpret_cast<const f32x4*>(Ds + rB * LR_LD + c4 * 4);
      const f32x4 x1 = *reinterpret_cast<const f32x4*>(Ds + (rB + 1) * LR_LD + c4 * 4);
#pragma unroll
      for (int kk = 0; kk < KG; ++kk) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(As + (kB0 + 8 * kk) * LR_LD + c4 * 4);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          accB[0][kk] = x0[c] * a[c] + accB[0][kk];
          accB[1][kk] = x1[c] * a[c] + accB[1][kk];
        }
      }
    }
  }
  float* db = out + d.db_off;
#pragma unroll
  for (int rr = 0; rr < 2; ++rr)
#pragma unroll
    for (int kk = 0; kk < KG; ++kk) {
      const long i = row0 + rB + rr;
      const int k = kB0 + 8 * kk;
      if (i < d.out && k < d.r) db[i * d.r + k] = d.s * accB[rr][kk];
    }
}

__global__ __launch_bounds__(256) void lora_grads_kernel(const LoraDesc* __restrict__ dglob, int nd, const float* __restrict__ grads,
                                                         float* __restrict__ out, float* __restrict__ slab) {
  extern __shared__ __attribute__((aligned(16))) char lr_smem[];
  LoraDesc* dsh = reinterpret_cast<LoraDesc*>(lr_smem);
  float* Bs = reinterpret_cast<float*>(lr_smem + (((size_t)nd * sizeof(LoraDesc) + 15) & ~(size_t)15));
  float* As = Bs + LR_BS;
  float* Ds = As + LR_TILE;
  const LoraDesc* tab = mt_stage_table(dsh, dglob, nd);
  const long total = tab[nd - 1].rb_prefix + lr_blocks(tab[nd - 1]);
  for (long u = blockIdx.x; u < total; u += gridDim.x) {
    const LoraDesc& d = tab[lr_find(tab, nd, u)];
    const long blk = u - d.rb_prefix;
    if (d.r <= 8) lr_grads_unit<8>(d, blk, grads, out, slab, Bs, As, Ds);
    else if (d.r <= 16) lr_grads_unit<16>(d, blk, grads, out, slab, Bs, As, Ds);
    else if (d.r <= 32) lr_grads_unit<32>(d, blk, grads, out, slab, Bs, As, Ds);
    else lr_grads_unit<64>(d, blk, grads, out, slab, Bs, As, Ds);
  }
}

// ---- gradients, launch 2: dA = s * (the tensor's partials added in block order) ----------------------------------------------------------
__global__ __launch_bounds__(256) void lora_da_reduce_kernel(const LoraDesc* __restrict__ dglob, int nd, const float* __restrict__ slab,
                                                             float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) char lr_smem[];
  TableWalker<LoraDesc> tw{mt_stage_table(reinterpret_cast<LoraDesc*>(lr_smem), dglob, nd), nd, 0};
  const LoraDesc& last = tw.d[nd - 1];
  const long total4 = last.n4_prefix + (long)last.r * last.in / 4;
  for (long g = (long)blockIdx.x * blockDim.x + threadIdx.x; g < total4; g += (long)gridDim.x * blockDim.x) {
    tw.seek(g);
    const LoraDesc& d = tw.cur();
    const long local = (g - d.n4_prefix) * 4, stride = (long)d.r * d.in;
    const float* p = slab + d.slab_off + local;
    const long nb = lr_blocks(d);
    f32x4 sum = {0.f, 0.f, 0.f, 0.f};
    long b = 0;
    for (; b + 4 <= nb; b += 4) {  // four loads in flight, added in block order
      f32x4 x[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) x[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p + (b + u) * stride));
#pragma unroll
      for (int u = 0; u < 4; ++u) sum = sum + x[u];
    }
    for (; b < nb; ++b) sum = sum + __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p + b * stride));
    *reinterpret_cast<f32x4*>(out + d.n4_prefix * 4 + local) = d.s * sum;
  }
}

constexpr size_t LR_MERGE_TILES = (size_t)(LR_BS + LR_TILE) * 4;
constexpr size_t LR_GRADS_TILES = (size_t)(LR_BS + 2 * LR_TILE) * 4;

}  // namespace
}  // namespace klab

using namespace klab;

extern "C" int klab_lora_merge(const void* desc_dev, int ndesc, void* arena, int dtype, int to_master, void* stream) {
  if (ndesc < 0 || (ndesc > 0 && !desc_dev) || (!to_master && !arena)) return KLAB_ERR_BADARG;
  if (!to_master && dtype != KLAB_BF16 && dtype != KLAB_F32) return KLAB_ERR_BADARG;
  if (ndesc > MT_MAXD) return KLAB_ERR_UNSUPPORTED;
  if (ndesc == 0) return KLAB_OK;
  const LoraDesc* tab = (const LoraDesc*)desc_dev;
  const size_t lds = lr_table_bytes(ndesc) + LR_MERGE_TILES, lds_max = lr_table_bytes(MT_MAXD) + LR_MERGE_TILES;
  auto go = [&](auto kern, auto* a) -> int {
    const int rc = ensure_dyn_lds(reinterpret_cast<const void*>(kern), lds_max);
    if (rc != KLAB_OK) return rc;
    hipLaunchKernelGGL(kern, dim3(LR_GRID), dim3(256), lds, (hipStream_t)stream, tab, ndesc, a);
    return KLAB_OK;
  };
  int rc;
  if (to_master) rc = go(lora_merge_kernel<float, true>, (float*)nullptr);
  else if (dtype == KLAB_BF16) rc = go(lora_merge_kernel<bf16_t, false>, (bf16_t*)arena);
  else rc = go(lora_merge_kernel<float, false>, (float*)arena);
  if (rc != KLAB_OK) return rc;
  KLAB_LAUNCH_CHECK();
  return KLAB_OK;
}

extern "C" int klab_lora_grads(const void* desc_dev, int ndesc, const float* grads, float* out, float* slab, void* stream) {
  if (ndesc < 0 || (ndesc > 0 && (!desc_dev || !grads || !out || !slab))) return KLAB_ERR_BADARG;
  if (ndesc > MT_MAXD) return KLAB_ERR_UNSUPPORTED;
  if (ndesc == 0) return KLAB_OK;
  const LoraDesc* tab = (const LoraDesc*)desc_dev;
  int rc = ensure_dyn_lds(reinterpret_cast<const void*>(lora_grads_kernel), lr_table_bytes(MT_MAXD) + LR_GRADS_TILES);
  if (rc != KLAB_OK) return rc;
  rc = ensure_dyn_lds(reinterpret_cast<const void*>(lora_da_reduce_kernel), lr_table_bytes(MT_MAXD));
  if (rc != KLAB_OK) return rc;
  hipLaunchKernelGGL(lora_grads_kernel, dim3(LR_GRID), dim3(256), lr_table_bytes(ndesc) + LR_GRADS_TILES, (hipStream_t)stream, tab, ndesc, grads,
                     out, slab);
  hipLaunchKernelGGL(lora_da_reduce_kernel, dim3(LR_GRID), dim3(256), lr_table_bytes(ndesc), (hipStream_t)stream, tab, ndesc,
                     (const float*)slab, out);
  KLAB_LAUNCH_CHECK();
  return KLAB_OK;
}

extern "C" int klab_lora_row_block(void) { return LR_ROWS; }
