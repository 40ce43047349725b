// Logits processors on the device (HF's `_get_logits_processor`, transformers/generation/utils.py, with the processors of
// generation/logits_process.py): RepetitionPenalty -> NoRepeatNGram -> NoBadWords -> MinLength -> MinNewTokensLength.
//
//   klab_logits_process_rows : one 1024-thread workgroup per row.  The row stays in registers (PROC_NPT = 32 consecutive tokens
//                              per thread, V <= PROC_THREADS * PROC_NPT), so thread t owns exactly the tokens of bit word t of
//                              two LDS bitmaps over the vocabulary:
//     1. scores = fp32 logits, or log_softmax of them (beam search scores log-probabilities: row max and sum-exp over the block);
//     2. the history (position 0 = the start token) goes to LDS; then, in parallel, one thread per history token sets its bit in
//        the penalty map, one thread per n-gram window start and one per bad-word entry set the bit of the token they ban in
//        the ban map, and EOS is banned by length;
//     3. every thread applies its own words: penalty first (from the original score, so a token repeated in the history is
//        penalised once, as HF's gather / scatter does), then -inf for the bans.  The bitmaps make the result independent of
//        the order in which the atomics land;
//     4. the dense fp32 row is written (optional in pick mode) and, in pick mode, the arg-max (lowest id among equal maxima) is
//        taken with klab_sample_rows' bookkeeping: pad after done, done on EOS, the sequence write and the stop word; on request
//        also the pick's log-probability under the processed row, log_softmax(s)[tok] (one more sum-exp reduction).
#include <math.h>

#include "common.h"
#include "klab_mm.h"
#include "row_regs.h"

namespace klab {

constexpr int PROC_MAX_HIST = 1024;  // cur_len

__global__ __launch_bounds__(PROC_THREADS) void logits_process_rows_kernel(klab_logits_proc_args a) {
  __shared__ uint32_t s_pen[PROC_THREADS], s_ban[PROC_THREADS];
  __shared__ int s_hist[PROC_MAX_HIST];
  __shared__ float s_f[2][PROC_WAVES];
  __shared__ int s_i[PROC_WAVES];
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int V = a.V, j0 = tid * PROC_NPT, L = a.cur_len;
  const int nv = max(0, min(PROC_NPT, V - j0));
  s_pen[tid] = 0u;
  s_ban[tid] = 0u;
  for (int p = tid; p < L; p += PROC_THREADS) s_hist[p] = p == 0 ? a.start_id : (int)a.seq[(long)r * a.ld_seq + p];
  // 1. scores (the padding slots past V hold -inf and are never written)
  float v[PROC_NPT];
  row_load(v, a.dtype, a.logits, (long)(r / a.row_div) * a.ld + j0, nv);
  if (a.log_softmax) row_log_softmax(v, nv, s_f);
  __syncthreads();  // the history and the cleared bitmaps
  // 2. the penalty map and the ban map
  if (a.repetition_penalty != 1.f) {
    for (int p = tid; p < L; p += PROC_THREADS) {
      const int t = s_hist[p];
      if (t >= 0 && t < V) atomicOr(&s_pen[t >> 5], 1u << (t & 31));
    }
  }
  const int n = a.no_repeat_ngram_size;
  if (n > 0 && L >= n) {
    const int tail = L - n + 1;  // the last n-1 tokens start here; windows start at 0 .. L-n
    for (int w = tid; w < tail; w += PROC_THREADS) {
      bool eq = true;
      for (int q = 0; q < n - 1 && eq; ++q) eq = s_hist[w + q] == s_hist[tail + q];
      const int t = s_hist[w + n - 1];
      if (eq && t >= 0 && t < V) atomicOr(&s_ban[t >> 5], 1u << (t & 31));
    }
  }
  for (int i = tid; i < a.n_bad; i += PROC_THREADS) {
    const int b0 = a.bad_off[i], len = a.bad_off[i + 1] - b0;
    if (len < 1 || len > L) continue;  // an entry longer than the history is ignored (HF: len(sequence_ids) > input_ids.shape[1])
    bool eq = true;
    for (int q = 0; q < len - 1 && eq; ++q) eq = s_hist[L - len + 1 + q] == a.bad_tok[b0 + q];
    const int t = a.bad_tok[b0 + len - 1];
    if (eq && t >= 0 && t < V) atomicOr(&s_ban[t >> 5], 1u << (t & 31));
  }
  if (tid == 0 && (L < a.min_length || L - 1 < a.min_new_tokens) && a.eos_id >= 0 && a.eos_id < V)
    atomicOr(&s_ban[a.eos_id >> 5], 1u << (a.eos_id & 31));
  __syncthreads();
  // 3. this thread's words: the penalty from the original score, then the bans
  const uint32_t pm = s_pen[tid], bm = s_ban[tid];
  const float pen = a.repetition_penalty;
#pragma unroll
  for (int c = 0; c < PROC_NPT; ++c) {
    if ((pm >> c) & 1u) v[c] = v[c] < 0.f ? v[c] * pen : v[c] / pen;
    if ((bm >> c) & 1u) v[c] = -INFINITY;
  }
  // 4. the dense row
  if (a.out) {
    row_store(v, a.out + (long)r * a.ld_out + j0, nv);
  }
  if (!a.pick) return;
  // arg-max: (value, id) ranks above when larger, or equal with the lower id; every thread starts from its own first token, so
  // a row of -inf picks 0
  float bv = nv > 0 ? v[0] : -INFINITY;
  int bi = nv > 0 ? j0 : INT_MAX;
#pragma unroll
  for (int c = 1; c < PROC_NPT; ++c)
    if (c < nv && v[c] > bv) { bv = v[c]; bi = j0 + c; }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float w = __shfl_xor(bv, o, 64);
    const int j = __shfl_xor(bi, o, 64);
    if (w > bv || (w == bv && j < bi)) { bv = w; bi = j; }
  }
  if (lane == 0) { s_f[0][wid] = bv; s_i[wid] = bi; }
  __syncthreads();
  // HF's transition score of the pick: log_softmax of the processed row at its arg-max = -log(sum exp(s - max)); the waves' maxima
  // are the row max, so the one extra reduction is the sum (s_f[1] is free since the log_softmax of step 1)
  if (a.logprob) {
    float M = s_f[0][0];
    for (int q = 1; q < PROC_WAVES; ++q) M = fmaxf(M, s_f[0][q]);
    float s = 0.f;
    if (M > -INFINITY) {
#pragma unroll
      for (int c = 0; c < PROC_NPT; ++c) s += expf(v[c] - M);  // (the padding slots and the bans hold -inf: 0)
    }
    s = wave_sum(s);
    if (lane == 0) s_f[1][wid] = s;
    __syncthreads();
  }
  if (tid != 0) return;
  for (int q = 1; q < PROC_WAVES; ++q)
    if (s_f[0][q] > bv || (s_f[0][q] == bv && s_i[q] < bi)) { bv = s_f[0][q]; bi = s_i[q]; }
  int tok = bi == INT_MAX ? 0 : bi;
  int fin = 0, was = 0;
  if (a.done) {
    fin = was = a.done[r];
    if (fin) tok = a.pad_id;
    else if (tok == a.eos_id) { fin = 1; a.done[r] = 1; }
  }
  if (a.logprob) {  // s[tok] is the row max: (s[tok] - max) - log(sum) = -log(sum); a row of -inf scores -inf, a row finished on entry 0
    float S = 0.f;
    for (int q = 0; q < PROC_WAVES; ++q) S += s_f[1][q];
    a.logprob[(long)r * a.ld_logprob + L] = was ? 0.f : bv > -INFINITY ? -logf(S) : -INFINITY;
  }
  if (a.tokens) a.tokens[r] = tok;
  if (a.seq) {
    a.seq[(long)r * a.ld_seq + L] = tok;
    if (L == 1) a.seq[(long)r * a.ld_seq] = a.start_id;
  }
  if (a.stop_word && !fin) *a.stop_word = 1;  // every writer stores the same value
}

}  // namespace klab

extern "C" int klab_logits_process_rows(const klab_logits_proc_args* a, void* stream) {
  using namespace klab;
  if (!a || !a->logits || a->rows <= 0 || a->V < 1 || a->row_div < 1 || a->ld < a->V || a->cur_len < 1 || !(a->repetition_penalty > 0.f) ||
      a->no_repeat_ngram_size < 0 || a->n_bad < 0 || (a->n_bad > 0 && (!a->bad_off || !a->bad_tok)) || (!a->out && !a->pick) ||
      (a->out && a->ld_out < a->V) || (a->cur_len > 1 && !a->seq) || (a->pick && a->seq && a->ld_seq <= a->cur_len) || (a->pick && a->logprob && a->ld_logprob <= a->cur_len) ||
      (a->seq && a->ld_seq < a->cur_len))
    return KLAB_ERR_BADARG;
  if (a->V > PROC_THREADS * PROC_NPT || a->cur_len > PROC_MAX_HIST) return KLAB_ERR_UNSUPPORTED;
  if (a->dtype != KLAB_F32 && a->dtype != KLAB_BF16) return KLAB_ERR_BADARG;
  hipLaunchKernelGGL(logits_process_rows_kernel, dim3(a->rows), dim3(PROC_THREADS), 0, (hipStream_t)stream, *a);
  KLAB_LAUNCH_CHECK();
  return KLAB_OK;
}
