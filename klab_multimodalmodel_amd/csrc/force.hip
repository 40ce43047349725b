// Forced decoding: the next token of every row comes from a table instead of being chosen (scoring given captions, decoder prompts).
//
//   klab_force_rows : position pos of every row, with the bookkeeping of klab_sample_rows / the pick of klab_logits_process_rows
//                     (done, pad after EOS, tokens, seq, stop word) and optionally the token's log-probability under the raw row.
//     logprob given : one FORCE_THREADS workgroup per row reads the row ONCE with 16-byte loads; every thread keeps an online
//                     (max, sum exp) pair, rescaled once per vector, merged across the wave and then across the waves in LDS
//                     (as ce_kernel and beam_topk_rows_kernel do); thread 0 gathers x[token] and writes
//                     (x[token] - M) - logf(S).  No register row, so no cap on V; no atomics.  A row finished on entry reads
//                     nothing and writes 0.
//     logprob NULL  : one thread per row, the logits are never touched (a prompt position needs none).
#include <math.h>

#include "common.h"
#include "klab_mm.h"

namespace klab {

constexpr int FORCE_THREADS = 512;
constexpr int FORCE_WAVES = FORCE_THREADS / 64;

// the token of row r (pad for a row finished on entry) and everything the choosing kernels write for it
__device__ __forceinline__ void force_book(const klab_force_args& a, int r, long long tok, int was) {
  int fin = was;
  if (was) tok = a.pad_id;
  else if (a.finish_on_eos && tok == a.eos_id) {
    fin = 1;
    if (a.done) a.done[r] = 1;
  }
  if (a.tokens) a.tokens[r] = tok;
  if (a.seq) {
    a.seq[(long)r * a.ld_seq + a.pos] = tok;
    if (a.pos == 1) a.seq[(long)r * a.ld_seq] = a.start_id;
  }
  if (a.stop_word && !fin) *a.stop_word = 1;  // every writer stores the same value
}

__global__ __launch_bounds__(256) void force_rows_plain_kernel(klab_force_args a) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= a.rows) return;
  force_book(a, r, a.forced[(long)r * a.ld_forced + a.pos], a.done ? a.done[r] : 0);
}

template <typename T>
__global__ __launch_bounds__(FORCE_THREADS) void force_rows_logprob_kernel(klab_force_args a) {
  __shared__ float s_m[FORCE_WAVES], s_s[FORCE_WAVES];
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int V = a.V;
  const int was = a.done ? a.done[r] : 0;  // (uniform over the workgroup; done[r] is written only behind the barrier below)
  const long long tok = a.forced[(long)r * a.ld_forced + a.pos];
  float* out = a.logprob + (long)r * a.ld_logprob + a.pos;
  if (was) {
    if (tid == 0) {
      *out = 0.f;
      force_book(a, r, tok, was);
    }
    return;
  }
  const T* x = (const T*)a.logits + (long)(r / a.row_div) * a.ld;
  float m = -INFINITY, s = 0.f;
  constexpr int VEC = 16 / sizeof(T);
  int j0 = 0;
  if ((V % VEC) == 0 && ((uintptr_t)x % 16) == 0) {
    for (int j = tid * VEC; j < V; j += FORCE_THREADS * VEC) {
      const typename Vec16<T>::type q = *reinterpret_cast<const typename Vec16<T>::type*>(x + j);
      float f[VEC], vm = -INFINITY;
#pragma unroll
      for (int c = 0; c < VEC; ++c) {
        f[c] = (float)q[c];
        vm = fmaxf(vm, f[c]);
      }
      if (vm > m) {  // (m == -inf: s is 0, and expf(-inf) = 0 keeps it)
        s *= expf(m - vm);
        m = vm;
      }
      if (m > -INFINITY) {
#pragma unroll
        for (int c = 0; c < VEC; ++c) s += expf(f[c] - m);
      }
    }
    j0 = V;
  }
  for (int j = j0 + tid; j < V; j += FORCE_THREADS) {
    const float v = to_f32(x[j]);
    if (v > m) {
      s = s * expf(m - v) + 1.f;
      m = v;
    } else if (m > -INFINITY) {
      s += expf(v - m);
    }
  }
  const float mw = wave_max(m);
  const float sw = wave_sum(m == -INFINITY ? 0.f : s * expf(m - mw));
  if (lane == 0) { s_m[wid] = mw; s_s[wid] = sw; }
  __syncthreads();
  if (tid != 0) return;
  float M = s_m[0];
  for (int w = 1; w < FORCE_WAVES; ++w) M = fmaxf(M, s_m[w]);
  float S = 0.f;
  for (int w = 0; w < FORCE_WAVES; ++w) S += s_m[w] == -INFINITY ? 0.f : s_s[w] * expf(s_m[w] - M);
  // a token outside the row reads nothing (the Python layer refuses such a table first)
  *out = (tok >= 0 && tok < V) ? (to_f32(x[tok]) - M) - logf(S) : -INFINITY;
  force_book(a, r, tok, was);
}

}  // namespace klab

extern "C" int klab_sizeof_force_args(void) { return (int)sizeof(klab_force_args); }

extern "C" int klab_force_rows(const klab_force_args* a, void* stream) {
  using namespace klab;
  if (!a || !a->forced || a->rows <= 0 || a->pos < 1 || a->ld_forced <= a->pos || (a->seq && a->ld_seq <= a->pos)) return KLAB_ERR_BADARG;
  hipStream_t s = (hipStream_t)stream;
  if (!a->logprob) {
    hipLaunchKernelGGL(force_rows_plain_kernel, dim3((a->rows + 255) / 256), dim3(256), 0, s, *a);
    KLAB_LAUNCH_CHECK();
    return KLAB_OK;
  }
  if (!a->logits || a->V < 1 || a->row_div < 1 || a->ld < a->V || a->ld_logprob <= a->pos) return KLAB_ERR_BADARG;
  if (a->dtype == KLAB_BF16) hipLaunchKernelGGL(force_rows_logprob_kernel<bf16_t>, dim3(a->rows), dim3(FORCE_THREADS), 0, s, *a);
  else if (a->dtype == KLAB_F32) hipLaunchKernelGGL(force_rows_logprob_kernel<float>, dim3(a->rows), dim3(FORCE_THREADS), 0, s, *a);
  else return KLAB_ERR_BADARG;
  KLAB_LAUNCH_CHECK();
  return KLAB_OK;
}
