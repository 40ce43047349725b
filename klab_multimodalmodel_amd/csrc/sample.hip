// Sampling on the device (HF's `_sample`, transformers/generation/utils.py, with the warpers of generation/logits_process.py).
//
//   klab_sample_rows : one 1024-thread workgroup per row turns a row of logits into one drawn token.  The row stays in registers
//                      (SAMPLE_NPT consecutive tokens per thread, V <= SAMPLE_THREADS * SAMPLE_NPT), and in one launch:
//     1. scores s = fp32 logits / temperature (HF's TemperatureLogitsWarper);
//     2. top-k: the k-th largest score by a radix select (4 passes of 8 bits, MSB first) over order-preserving uint32 keys;
//        every score >= it is kept, so ties at the k-th value are kept, as HF's TopKLogitsWarper does;
//     3. top-p: p = softmax of the top-k-kept scores.  Token i stays iff the mass of the kept tokens with a STRICTLY larger score
//        is < top_p (the arg-max always stays).  A second radix select over the same keys, weighted by mass, finds the smallest
//        key that satisfies it.  This is HF's ascending-sort-and-cumsum rule except among tokens that tie exactly at the
//        boundary: HF's sort order splits such a tie, this kernel keeps the whole tie group;
//     4. draw: over the kept tokens in ascending token id, the smallest id j whose running sum of kept probability exceeds
//        u * (sum of kept probability), with u in [0, 1) from sample_uniform(seed, step, row) below (or given by the caller);
//     5. greedy's bookkeeping: a finished row (done[r]) draws pad; EOS sets done[r]; the token goes to tokens[r] and
//        seq[r, pos]; stop_word = 1 while any row is unfinished.
//     6. optionally the token's log-probability under the processed scores, log_softmax(s)[tok] = (s[tok] - M) - log G with the
//        row max M and the kept mass G of step 4 (HF's compute_transition_scores(normalize_logits=True)); 0 for a finished row.
//   klab_gen_finalize : one wave per image over the per-token log-probabilities of a finished session: each row's length (through
//                       its first EOS), its score sum / length^length_penalty (beam search's convention), and the rows of the
//                       image ranked by score (counting rank, ties to the lower row).
//   The histograms live in LDS, replicated SAMPLE_REP times (lane % SAMPLE_REP; a 257-entry stride puts replicas on different
//   banks) so that the many scores that share a top byte do not serialise on one address.  Counts and masses are integers
//   (mass in units of 2^-40 in the upper 48 bits, count in the lower 16 of one uint64), so the result does not depend on the
//   order in which the atomics land: the same inputs draw the same token on every run.
#include <math.h>

#include "common.h"
#include "klab_mm.h"

namespace klab {

constexpr int SAMPLE_THREADS = 1024;
constexpr int SAMPLE_NPT = 32;  // logits per thread: V <= 32768
constexpr int SAMPLE_REP = 16;
constexpr int SAMPLE_BINS = 256;
constexpr int SAMPLE_HSTRIDE = SAMPLE_BINS + 1;
constexpr int SAMPLE_WAVES = SAMPLE_THREADS / 64;
constexpr float SAMPLE_MASS_ONE = 1099511627776.0f;  // 2^40

// order-preserving map of a float to uint32 (larger float -> larger key; -inf -> 0x007FFFFF).  The slots past V hold key 0,
// below every score's: "key >= lo" with lo >= 1 is also the bounds check.
__device__ __forceinline__ uint32_t sample_key(float x) {
  const uint32_t b = __float_as_uint(x);
  return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float sample_val(uint32_t k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu)); }

// u in [0, 1) (24 bits) from (seed, step, row): four rounds of mix32 (common.h) over the seed words, the step and the row
__device__ __forceinline__ float sample_uniform(unsigned long long seed, int step, int row) {
  uint32_t h = mix32((uint32_t)seed * 0x9E3779B1u + 0x7FEB352Du);
  h = mix32(h ^ ((uint32_t)(seed >> 32) * 0x85EBCA77u + 0x165667B1u));
  h = mix32(h ^ ((uint32_t)step * 0xC2B2AE3Du + 0x27D4EB2Fu));
  h = mix32(h ^ ((uint32_t)row * 0x9E3779B1u + 0x85EBCA6Bu));
  return (float)(h >> 8) * (1.0f / 16777216.0f);
}

__device__ __forceinline__ unsigned long long shfl_up_u64(unsigned long long v, int o) {
  const uint32_t lo = __shfl_up((uint32_t)v, o, 64), hi = __shfl_up((uint32_t)(v >> 32), o, 64);
  return ((unsigned long long)hi << 32) | lo;
}

// One MSB-first radix select over the keys of the elements with key >= lo (>= 1).  Each element weighs (mass << 16) | 1, its mass
// round(e * inv[0] * 2^40) (top-p) or 0 (top-k).  (inv is re-read from LDS every pass, so the compiler does not keep all the
// weights live across the passes.)
//   TOPP = false: returns the key of the k-th largest element (k = target, 1 <= k <= number of elements).
//   TOPP = true : returns the smallest key t such that the mass of the elements with key > t is < target (target >= 1).
template <bool TOPP>
__device__ uint32_t radix_select(const uint32_t (&k)[SAMPLE_NPT], const float (&e)[SAMPLE_NPT], const float* inv, uint32_t lo,
                                 unsigned long long target, unsigned long long* hist, unsigned long long* red, uint32_t* sel) {
  const int tid = threadIdx.x, lane = tid & 63, rep = lane % SAMPLE_REP;
  uint32_t prefix = 0;
  unsigned long long above = 0;  // count (top-k) or mass (top-p) of the elements above the current prefix's range
  for (int level = 0; level < 4; ++level) {
    const int shift = 24 - 8 * level;
    for (int i = tid; i < SAMPLE_REP * SAMPLE_HSTRIDE; i += SAMPLE_THREADS) hist[i] = 0;
    __syncthreads();
    const float sc = TOPP ? inv[0] * SAMPLE_MASS_ONE : 0.f;
#pragma unroll
    for (int c = 0; c < SAMPLE_NPT; ++c) {
      const uint32_t key = k[c];
      const bool in = key >= lo && (level == 0 || (key >> (shift + 8)) == (prefix >> (shift + 8)));
      const unsigned long long w = TOPP ? ((unsigned long long)(e[c] * sc + 0.5f) << 16) | 1ull : 1ull;
      if (in) atomicAdd(&hist[rep * SAMPLE_HSTRIDE + ((key >> shift) & 255)], w);
    }
    __syncthreads();
    // bin b = tid / TPB: the sum over the replicas (TPB neighbouring threads per bin, REP / TPB replicas each)
    {
      constexpr int TPB = SAMPLE_THREADS / SAMPLE_BINS, RPT = SAMPLE_REP / TPB;
      const int b = tid / TPB, r0 = (tid % TPB) * RPT;
      unsigned long long v = 0;
#pragma unroll
      for (int r = 0; r < RPT; ++r) v += hist[(r0 + r) * SAMPLE_HSTRIDE + b];
#pragma unroll
      for (int o = 1; o < TPB; o <<= 1) {
        const uint32_t lo32 = __shfl_xor((uint32_t)v, o, 64), hi32 = __shfl_xor((uint32_t)(v >> 32), o, 64);
        v += ((unsigned long long)hi32 << 32) | lo32;
      }
      if (tid % TPB == 0) red[b] = v;
    }
    __syncthreads();
    if (tid < 64) {
      // lane l holds bins 255-4l .. 252-4l (descending); exclusive prefix over the lanes of the descending totals
      unsigned long long v[4], tot = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) { v[q] = red[255 - 4 * lane - q]; tot += TOPP ? (v[q] >> 16) : (v[q] & 0xFFFF); }
      unsigned long long inc = tot;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long t = shfl_up_u64(inc, o);
        if (lane >= o) inc += t;
      }
      unsigned long long before = above + inc - tot;
      int pick = -1;
      unsigned long long pick_before = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const unsigned long long cnt = v[q] & 0xFFFF, m = TOPP ? (v[q] >> 16) : cnt;
        if (TOPP) {
          if (cnt > 0 && before < target) { pick = q; pick_before = before; }  // the lowest such bin
        } else {
          if (pick < 0 && before < target && before + cnt >= target) { pick = q; pick_before = before; }
        }
        before += m;
      }
      const unsigned long long ball = __ballot(pick >= 0);
      const int src = TOPP ? 63 - __builtin_clzll(ball) : __builtin_ctzll(ball);  // top-p: the last lane (lowest bins)
      if (lane == src) {
        sel[0] = (uint32_t)(255 - 4 * lane - pick);
        sel[1] = (uint32_t)pick_before;
        sel[2] = (uint32_t)(pick_before >> 32);
      }
    }
    __syncthreads();
    prefix |= sel[0] << shift;
    above = ((unsigned long long)sel[2] << 32) | sel[1];
    __syncthreads();  // sel and red are rewritten by the next level
  }
  return prefix;
}

template <typename T>
__global__ __launch_bounds__(SAMPLE_THREADS) void sample_rows_kernel(klab_sample_args a) {
  __shared__ unsigned long long s_hist[SAMPLE_REP * SAMPLE_HSTRIDE];
  __shared__ unsigned long long s_red[SAMPLE_BINS];
  __shared__ float s_f[SAMPLE_WAVES], s_inv;
  __shared__ uint32_t s_sel[3];
  __shared__ int s_pick[SAMPLE_WAVES];
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int V = a.V, j0 = tid * SAMPLE_NPT;
  const int nv = max(0, min(SAMPLE_NPT, V - j0));
  const T* x = (const T*)a.logits + (long)(r / a.row_div) * a.ld + j0;
  uint32_t k[SAMPLE_NPT];  // keys of the scores (sample_key); the padding slots past V hold key 0
  // 1. scores (fp32 logits / temperature, a true division as HF's `scores / self.temperature`) and the row max (the arg-max is
  //    kept by both warpers)
  const float temp = a.temperature;
  float m = -INFINITY;
  constexpr int VEC = 16 / sizeof(T);
  if (nv == SAMPLE_NPT && ((uintptr_t)x % 16) == 0) {
#pragma unroll
    for (int c = 0; c < SAMPLE_NPT; c += VEC) {
      const typename Vec16<T>::type q = *reinterpret_cast<const typename Vec16<T>::type*>(x + c);
#pragma unroll
      for (int t = 0; t < VEC; ++t) {
        const float v = (float)q[t] / temp;
        m = fmaxf(m, v);
        k[c + t] = sample_key(v);
      }
    }
  } else {
#pragma unroll
    for (int c = 0; c < SAMPLE_NPT; ++c) {
      const float v = c < nv ? to_f32(x[c]) / temp : -INFINITY;
      m = fmaxf(m, v);
      k[c] = c < nv ? sample_key(v) : 0u;
    }
  }
  m = wave_max(m);
  if (lane == 0) s_f[wid] = m;
  __syncthreads();
  float M = s_f[0];
  for (int q = 1; q < SAMPLE_WAVES; ++q) M = fmaxf(M, s_f[q]);
  __syncthreads();
  float e[SAMPLE_NPT];
  // 2. top-k
  uint32_t lo = 1;
  if (a.top_k > 0 && a.top_k < V) lo = radix_select<false>(k, e, nullptr, 1, (unsigned long long)a.top_k, s_hist, s_red, s_sel);
  // 3. top-p over the softmax of the top-k-kept scores
  float z = 0.f;
#pragma unroll
  for (int c = 0; c < SAMPLE_NPT; ++c) {
    e[c] = k[c] >= lo ? expf(sample_val(k[c]) - M) : 0.f;
    z += e[c];
  }
  z = wave_sum(z);
  if (lane == 0) s_f[wid] = z;
  __syncthreads();
  if (tid == 0) {
    float Z = 0.f;
    for (int q = 0; q < SAMPLE_WAVES; ++q) Z += s_f[q];
    s_inv = 1.f / Z;
  }
  __syncthreads();
  if (a.top_p < 1.f) {
    unsigned long long target = (unsigned long long)((double)a.top_p * (double)SAMPLE_MASS_ONE);
    if (target < 1) target = 1;  // top_p = 0: only the arg-max group (mass above it is 0)
    const uint32_t tp = radix_select<true>(k, e, &s_inv, lo, target, s_hist, s_red, s_sel);
    lo = max(lo, tp);
  }
  // the processed scores HF's `_sample` hands to softmax
  float ts = 0.f;
#pragma unroll
  for (int c = 0; c < SAMPLE_NPT; ++c) {
    if (k[c] < lo) e[c] = 0.f;
    ts += e[c];
  }
  if (a.warped) {
    float* o = a.warped + (long)r * a.ld_warped + j0;
    if (nv == SAMPLE_NPT && ((uintptr_t)o % 16) == 0) {
#pragma unroll
      for (int c = 0; c < SAMPLE_NPT; c += 4) {
        f32x4 q;
#pragma unroll
        for (int t = 0; t < 4; ++t) q[t] = k[c + t] >= lo ? sample_val(k[c + t]) : -INFINITY;
        *reinterpret_cast<f32x4*>(o + c) = q;
      }
    } else {
#pragma unroll
      for (int c = 0; c < SAMPLE_NPT; ++c)
        if (c < nv) o[c] = k[c] >= lo ? sample_val(k[c]) : -INFINITY;
    }
  }
  // 4. draw: exclusive scan of the per-thread kept mass in token order (threads own consecutive token ranges).  The exclusive
  //    value is the previous lane's inclusive one, not inc - ts: behind kept tokens of negligible mass the difference cancels to
  //    0 in the thread that holds the row's mass, which then looks like the first one and takes a u = 0 draw from them
  float inc = ts;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  if (lane == 63) s_f[wid] = inc;
  const float prev = __shfl_up(inc, 1, 64);
  __syncthreads();
  float base = lane ? prev : 0.f, G = 0.f;
  for (int q = 0; q < SAMPLE_WAVES; ++q) {
    if (q < wid) base += s_f[q];
    G += s_f[q];
  }
  const float u = a.u_in ? a.u_in[r] : sample_uniform(a.seed, a.step, r);
  const float target = u * G;
  // the thread of the crossing: the last one with kept mass whose base is <= target (the first kept token's base is 0)
  const bool cand = ts > 0.f && base <= target;
  const unsigned long long ball = __ballot(cand);
  if (lane == 0) s_pick[wid] = ball ? wid * 64 + 63 - __builtin_clzll(ball) : -1;
  __syncthreads();
  int owner = -1;
  for (int q = 0; q < SAMPLE_WAVES; ++q) owner = max(owner, s_pick[q]);
  if (tid != owner) return;
  int tok = -1, last = -1;
  float run = base;
#pragma unroll
  for (int c = 0; c < SAMPLE_NPT; ++c) {
    if (e[c] > 0.f) {
      run += e[c];
      last = c;
      if (tok < 0 && run > target) tok = c;
    }
  }
  const int ct = tok >= 0 ? tok : last;  // (rounding: the crossing fell past this thread's own sum -> its last kept token)
  tok = j0 + ct;
  // 5. bookkeeping
  int fin = 0, was = 0;
  if (a.done) {
    fin = was = a.done[r];
    if (fin) tok = a.pad_id;
    else if (tok == a.eos_id) { fin = 1; a.done[r] = 1; }
  }
  // HF's transition score of the draw: log_softmax of the processed row at the token, from the max and the kept mass the draw
  // used (a row finished on entry draws a forced pad: 0)
  if (a.logprob) {
    uint32_t kt = 0;
#pragma unroll
    for (int c = 0; c < SAMPLE_NPT; ++c)
      if (c == ct) kt = k[c];
    a.logprob[(long)r * a.ld_logprob + a.pos] = was ? 0.f : (sample_val(kt) - M) - logf(G);
  }
  if (a.tokens) a.tokens[r] = tok;
  if (a.seq) {
    a.seq[(long)r * a.ld_seq + a.pos] = tok;
    if (a.pos == 1) a.seq[(long)r * a.ld_seq] = a.start_id;
  }
  if (a.stop_word && !fin) *a.stop_word = 1;  // every writer stores the same value
}

// lane j of block b owns row b*n + j: one thread sums its row in ascending position (fp32, no atomics: the same inputs give the
// same bits), then the wave ranks the n scores by counting
__global__ __launch_bounds__(64) void gen_finalize_kernel(const float* __restrict__ logprob, long ld, const long long* __restrict__ seq,
                                                          long ld_seq, int n, int length, int eos_id, float length_penalty, int n_out,
                                                          float* __restrict__ score, int* __restrict__ len, int* __restrict__ order) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const long r = (long)b * n + lane;
  float sc = -INFINITY;
  if (lane < n) {
    int l = length - 1;
    float sum = 0.f;
    for (int p = 1; p < length; ++p) {
      sum += logprob[r * ld + p];
      if (seq[r * ld_seq + p] == eos_id) { l = p; break; }
    }
    sc = sum / powf((float)l, length_penalty);
    if (score) score[r] = sc;
    if (len) len[r] = l;
  }
  if (!order) return;
  int rank = 0;
  for (int i = 0; i < n; ++i) {
    const float o = __shfl(sc, i, 64);
    rank += (o > sc || (o == sc && i < lane)) ? 1 : 0;
  }
  if (lane < n && rank < n_out) order[(long)b * n_out + rank] = (int)r;
}

}  // namespace klab

extern "C" int klab_gen_finalize(const float* logprob, long ld, const long long* seq, long ld_seq, int B, int n, int length, int eos_id,
                                 float length_penalty, int n_out, float* score, int* len, int* order, void* stream) {
  using namespace klab;
  if (!logprob || !seq || B < 1 || n < 1 || length < 2 || ld < length || ld_seq < length || (order && (n_out < 1 || n_out > n)))
    return KLAB_ERR_BADARG;
  if (n > 64) return KLAB_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(gen_finalize_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, logprob, ld, seq, ld_seq, n, length, eos_id,
                     length_penalty, n_out, score, len, order);
  KLAB_LAUNCH_CHECK();
  return KLAB_OK;
}

extern "C" int klab_sample_rows(const klab_sample_args* a, void* stream) {
  using namespace klab;
  if (!a || !a->logits || a->rows <= 0 || a->V < 1 || a->row_div < 1 || a->ld < a->V || !(a->temperature > 0.f) || a->top_k < 0 ||
      !(a->top_p >= 0.f && a->top_p <= 1.f) || (a->warped && a->ld_warped < a->V) || (a->seq && (a->pos < 1 || a->ld_seq <= a->pos)) ||
      (a->logprob && (a->pos < 1 || a->ld_logprob <= a->pos)))
    return KLAB_ERR_BADARG;
  if (a->V > SAMPLE_THREADS * SAMPLE_NPT) return KLAB_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  if (a->dtype == KLAB_BF16) hipLaunchKernelGGL(sample_rows_kernel<bf16_t>, dim3(a->rows), dim3(SAMPLE_THREADS), 0, s, *a);
  else if (a->dtype == KLAB_F32) hipLaunchKernelGGL(sample_rows_kernel<float>, dim3(a->rows), dim3(SAMPLE_THREADS), 0, s, *a);
  else return KLAB_ERR_BADARG;
  KLAB_LAUNCH_CHECK();
  return KLAB_OK;
}
