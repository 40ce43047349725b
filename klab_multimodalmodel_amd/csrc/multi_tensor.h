// Multi-tensor kernels: ONE launch over many tensors, whatever their number.  The engine builds a descriptor table per kernel
// family at bind time (engine.cpp, klab_engine_bind) from the structs below; the kernels (misc.hip: cast_pack, adamw.hip: Adam
// and AdamW, ema.hip, gemm.hip: the fp8 weight quantiser, adafactor.hip) read exactly these structs.  LoraDesc tables (lora.hip) are
// the caller's: Python fills them from klab_engine_lora_layout.
//
// The vec4 walkers (cast_pack, Adam, AdamW, EMA) see the tensors as one space of 16-byte vectors: descriptor i owns the vec4
// indices [n4_prefix[i], n4_prefix[i + 1]).  A thread handles U vec4s a block width apart (every wave instruction is a contiguous
// 1 KiB access) and has all U loads of every stream in flight before any arithmetic.  Measured on the way here:
//  - a binary search per vec4 was 7 dependent loads in front of every 16-byte read: 2.4 TB/s.  So ONE search per thread and
//    iteration (TableWalker::seek), then a walk forward (advance); tensors are far longer than U * 256 vec4s.
//  - the search is a chain of DEPENDENT loads (eight for ~130 tensors, then three more per vector for the tensor's addresses).
//    From global memory that chain (~1.5 us of L2 round trips) ran in front of every batch of streaming loads and kept the
//    Adam step at 4.5 TB/s; a copy of the table in LDS makes it ~100 cycles per step.  Tables above MT_MAXD entries are read
//    from global memory.
//  - Adam with an 8-deep unroll measured 1.5 ms against ~0.4 (spills): U = 4 (MT_U) for the optimizer and EMA kernels, launched
//    as at most 1024 workgroups (4 per CU); cast_pack, with one stream in and one out, keeps U = 8.
//  - non-temporal loads / stores in the optimizer and EMA kernels: every byte is touched once per step (Adam: 415 -> 397 us).
#pragma once
#include "common.h"

namespace klab {

struct CastDesc { const float* src; long dst_off; long n4_prefix; };  // dst_off in elements of the destination arena
struct AdamDesc { float* p; long goff; long aoff; long n4_prefix; };   // goff: flat gradient buffer; aoff < 0: no arena copy
// klab_mm.h (klab_engine_adafactor_layout): 10 longs per tensor, read as such by Python
struct AfDesc { float* p; long goff, aoff, rows, cols, soff, tile0, tile_len, poff, factored; };
struct QuantDesc { long off; long rows; long K; long row0; };  // {arena element offset, rows, K, first global row}
// One LoRA target W [out, in] with A [r, in], B [out, r] and s = alpha / r (lora.hip; 11 longs per tensor to Python, {out, in} and
// {r, s} sharing one each).  aoff: arena copy, goff: dW in the flat gradient buffer.  n4_prefix: prefix sum of r * in / 4 -- dA lies
// at out[4 * n4_prefix], dB at out[db_off].  rb_prefix: prefix sum of the tensors' row blocks (ceil(out / klab_lora_row_block())),
// slab_off: the tensor's dA partials [row blocks, r, in] in the caller's slab.  in % 4 == 0, 1 <= r <= 64.
struct LoraDesc { float* w; const float* a; const float* b; long aoff, goff; int out, in; int r; float s; long n4_prefix, rb_prefix, slab_off, db_off; };
// n4_prefix is in units of 4 elements everywhere
static_assert(sizeof(LoraDesc) == 88, "eleven longs per tensor");
static_assert(sizeof(CastDesc) == 24 && sizeof(AdamDesc) == 32 && sizeof(AfDesc) == 80 && sizeof(QuantDesc) == 32,
              "the tables are arrays of longs to the engine's device buffers and to Python");

constexpr int MT_MAXD = 1024;  // table capacity in LDS (T5-large: ~560 tensors; 32 KiB of AdamDesc)
constexpr int MT_U = 4;

// Copies the table into the caller's __shared__ dsh[MT_MAXD] when it fits and returns the table to read.  Ends in a barrier
// either way, so whatever else the caller staged in LDS before the call is visible after it.
template <typename D>
__device__ __forceinline__ const D* mt_stage_table(D* dsh, const D* __restrict__ dglob, int nd) {
  const bool in_lds = nd <= MT_MAXD;
  if (in_lds)
    for (int i = threadIdx.x; i < nd; i += blockDim.x) dsh[i] = dglob[i];
  __syncthreads();
  return in_lds ? dsh : dglob;
}

template <typename D>
struct TableWalker {
  const D* d; int nd; int lo;
  __device__ __forceinline__ void seek(long g0) {  // lo = last descriptor with prefix <= g0
    lo = 0;
    int hi = nd - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (d[mid].n4_prefix <= g0) lo = mid; else hi = mid - 1;
    }
  }
  __device__ __forceinline__ const D& cur() const { return d[lo]; }
  // forward to the descriptor of vec4 g (>= the last g seen): cur() is that descriptor, the result the element offset inside it
  __device__ __forceinline__ long advance(long g) {
    while (lo + 1 < nd && d[lo + 1].n4_prefix <= g) ++lo;
    return (g - d[lo].n4_prefix) * 4;
  }
};

// one vec4 into an arena of T: bf16 round-to-nearest-even, or the f32 bits
template <typename T>
__device__ __forceinline__ void mt_store_vec4(T* dst, f32x4 v) {
  if constexpr (sizeof(T) == 2) *reinterpret_cast<bf16x4*>(dst) = bf16x4{(bf16_t)v[0], (bf16_t)v[1], (bf16_t)v[2], (bf16_t)v[3]};
  else *reinterpret_cast<f32x4*>(dst) = v;
}

inline unsigned mt_grid(long n4) {  // workgroups of 256 threads x MT_U vec4s, grid-stride above 1024
  const long gl = ((n4 + MT_U - 1) / MT_U + 255) / 256;
  return (unsigned)(gl < 1 ? 1 : (gl > 1024 ? 1024 : gl));
}

// f(arena as bf16_t* or float*): the caller has checked dtype
template <typename F>
inline void mt_dispatch(int dtype, void* arena, F&& f) {
  if (dtype == KLAB_BF16) f((bf16_t*)arena);
  else f((float*)arena);
}

}  // namespace klab
