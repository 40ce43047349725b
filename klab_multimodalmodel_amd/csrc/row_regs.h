// One vocabulary row in the registers of a 1024-thread workgroup: thread t owns the PROC_NPT = 32 consecutive tokens of bit word t of
// an LDS bitmap over the vocabulary.  Shared by klab_logits_process_rows (logits_proc.hip) and klab_constrain_rows (constrain.hip),
// whose log_softmax therefore is one piece of code: beam search scores the same bits behind either.
#pragma once
#include <math.h>

#include "common.h"

namespace klab {

constexpr int PROC_THREADS = 1024;
constexpr int PROC_NPT = 32;  // scores per thread = bits per bitmap word: V <= 32768
constexpr int PROC_WAVES = PROC_THREADS / 64;

// v[c] = the fp32 value of element off + c of base (dtype f32 or bf16) for c < nv, -inf in the padding slots past V
__device__ __forceinline__ void row_load(float (&v)[PROC_NPT], int dtype, const void* base, long off, int nv) {
  if (dtype == KLAB_F32) {
    const float* x = (const float*)base + off;
    if (nv == PROC_NPT && ((uintptr_t)x % 16) == 0) {
#pragma unroll
      for (int c = 0; c < PROC_NPT; c += 4) {
        const f32x4 q = *reinterpret_cast<const f32x4*>(x + c);
#pragma unroll
        for (int t = 0; t < 4; ++t) v[c + t] = q[t];
      }
    } else {
#pragma unroll
      for (int c = 0; c < PROC_NPT; ++c) v[c] = c < nv ? x[c] : -INFINITY;
    }
  } else {
    const bf16_t* x = (const bf16_t*)base + off;
    if (nv == PROC_NPT && ((uintptr_t)x % 16) == 0) {
#pragma unroll
      for (int c = 0; c < PROC_NPT; c += 8) {
        const bf16x8 q = *reinterpret_cast<const bf16x8*>(x + c);
#pragma unroll
        for (int t = 0; t < 8; ++t) v[c + t] = (float)q[t];
      }
    } else {
#pragma unroll
      for (int c = 0; c < PROC_NPT; ++c) v[c] = c < nv ? (float)x[c] : -INFINITY;
    }
  }
}

// v -> log_softmax(v) over the whole row: row max and sum-exp over the block (s_f: [2][PROC_WAVES] of LDS; two barriers, called by
// every thread of the block)
__device__ __forceinline__ void row_log_softmax(float (&v)[PROC_NPT], int nv, float (*s_f)[PROC_WAVES]) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  float m = -INFINITY;
#pragma unroll
  for (int c = 0; c < PROC_NPT; ++c) m = fmaxf(m, v[c]);
  m = wave_max(m);
  if (lane == 0) s_f[0][wid] = m;
  __syncthreads();
  float M = s_f[0][0];
  for (int q = 1; q < PROC_WAVES; ++q) M = fmaxf(M, s_f[0][q]);
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < PROC_NPT; ++c) s += c < nv ? expf(v[c] - M) : 0.f;
  s = wave_sum(s);
  if (lane == 0) s_f[1][wid] = s;
  __syncthreads();
  float S = 0.f;
  for (int q = 0; q < PROC_WAVES; ++q) S += s_f[1][q];
  const float logS = logf(S);
#pragma unroll
  for (int c = 0; c < PROC_NPT; ++c) v[c] = (v[c] - M) - logS;
}

// o[c] = v[c] for c < nv (o = the output row's element j0); columns past V are never written
__device__ __forceinline__ void row_store(const float (&v)[PROC_NPT], float* o, int nv) {
  if (nv == PROC_NPT && ((uintptr_t)o % 16) == 0) {
#pragma unroll
    for (int c = 0; c < PROC_NPT; c += 4) {
      f32x4 q;
#pragma unroll
      for (int t = 0; t < 4; ++t) q[t] = v[c + t];
      *reinterpret_cast<f32x4*>(o + c) = q;
    }
  } else {
#pragma unroll
    for (int c = 0; c < PROC_NPT; ++c)
      if (c < nv) o[c] = v[c];
  }
}

}  // namespace klab
