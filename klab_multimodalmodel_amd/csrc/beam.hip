// Beam-search decoding on the device (HF's vectorised `_beam_search`, transformers/generation/utils.py).
//
//   klab_beam_topk   : log_softmax of every row of logits [B*k, V] + the running score of that beam, then the 2k best
//                      (score, flat index = beam*V + token) of each sample over its k*V candidates, sorted descending.
//                      Two launches: one 256-thread workgroup per row streams the row once (online max / sum-exp and a
//                      per-thread sorted candidate list, merged across the workgroup in LDS), then one wave per sample merges
//                      the k sorted row lists.  Ties are broken by the LOWER flat index, in both stages.
//   klab_beam_topk_scores : the same over rows that already hold processed log-probabilities (csrc/logits_proc.hip); candidates are
//                      ranked by row + running score as f32 rounds it, so scores the add makes equal tie by the lower index too.
//   klab_beam_update : one wave per sample; HF's `_get_running_beams_for_next_iteration`, `_update_finished_beams`,
//                      `_check_early_stop_heuristic` and the per-sample part of `_beam_search_has_unfinished_sequences`
//                      over fixed-shape state (klab_beam_update_args, include/klab_mm.h).
//   klab_beam_init   : the state before HF's first step.
//   klab_beam_copy_rows : row replication used by the engine's beam_begin (position-0 self K/V of every beam).
#include <math.h>

#include "common.h"
#include "klab_mm.h"

namespace klab {

// threads per row workgroup: 256, or 128 for the 32-entry lists (the per-thread lists are staged in LDS)
template <int KMAX> constexpr int topk_threads() { return KMAX >= 32 ? 128 : 256; }

// (v, i) ranks above (w, j): larger score, or equal score and lower index
__device__ __forceinline__ bool beam_better(float v, int i, float w, int j) { return v > w || (v == w && i < j); }

__device__ __forceinline__ void wave_argmax(float& v, int& i) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float w = __shfl_xor(v, o, 64);
    const int j = __shfl_xor(i, o, 64);
    if (beam_better(w, j, v, i)) { v = w; i = j; }
  }
}

template <int KMAX>
__device__ __forceinline__ void list_insert(float (&lv)[KMAX], int (&li)[KMAX], float x, int ix) {
  if (!beam_better(x, ix, lv[KMAX - 1], li[KMAX - 1])) return;
  float cv = x;
  int ci = ix;
#pragma unroll
  for (int c = 0; c < KMAX; ++c) {
    if (beam_better(cv, ci, lv[c], li[c])) {
      const float tv = lv[c]; const int ti = li[c];
      lv[c] = cv; li[c] = ci; cv = tv; ci = ti;
    }
  }
}

// one workgroup per row r = b*k + beam: the K2 best (log_softmax(row) + run_score[r], beam*V + token) of the row, sorted.
// NORMED: the row already holds log-probabilities (f32, processed; may hold -inf): row + run_score[r], no log_softmax.
template <typename T, int KMAX, bool NORMED = false, int TOPK_THREADS = topk_threads<KMAX>()>
__global__ __launch_bounds__(TOPK_THREADS) void beam_topk_rows_kernel(const T* __restrict__ logits, long ld, int row_div,
                                                                     const float* __restrict__ run_score, int k, int V, int K2,
                                                                     float* __restrict__ row_score, int* __restrict__ row_idx) {
  __shared__ float s_v[TOPK_THREADS * KMAX];
  __shared__ int s_i[TOPK_THREADS * KMAX];
  __shared__ float s_red[2][TOPK_THREADS / 64];
  __shared__ int s_redi[2][TOPK_THREADS / 64];
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const T* x = logits + (long)(r / row_div) * ld;
  float lv[KMAX];
  int li[KMAX];
#pragma unroll
  for (int c = 0; c < KMAX; ++c) { lv[c] = -INFINITY; li[c] = INT_MAX; }
  float m = -INFINITY, s = 0.f;
  const float rs = run_score[r];
  // NORMED ranks by the final score row[j] + run_score[r], not by row[j]: the add can round distinct scores to one value (every
  // score of a -1e9 beam does), and such candidates tie by the lower index like any others.  (The log-softmax form ranks a row by
  // its logits: equal logits are the ties it orders by index.)
  auto take = [&](float xv, int j) {
    if constexpr (!NORMED) {
      if (xv > m) { s = s * __expf(m - xv) + 1.f; m = xv; }
      else s += __expf(xv - m);
      list_insert<KMAX>(lv, li, xv, j);
    } else {
      list_insert<KMAX>(lv, li, xv + rs, j);
    }
  };
  constexpr int VEC = 16 / sizeof(T);
  int j0 = 0;
  if ((V % VEC) == 0 && ((uintptr_t)x % 16) == 0) {
    for (int j = tid * VEC; j < V; j += TOPK_THREADS * VEC) {
      float f[VEC];
      if constexpr (sizeof(T) == 2) {
        const bf16x8 q = *reinterpret_cast<const bf16x8*>(x + j);
#pragma unroll
        for (int c = 0; c < VEC; ++c) f[c] = (float)q[c];
      } else {
        const f32x4 q = *reinterpret_cast<const f32x4*>(x + j);
#pragma unroll
        for (int c = 0; c < VEC; ++c) f[c] = q[c];
      }
#pragma unroll
      for (int c = 0; c < VEC; ++c) take(f[c], j + c);
    }
    j0 = V;
  }
  for (int j = j0 + tid; j < V; j += TOPK_THREADS) take(to_f32(x[j]), j);
  // row max and sum-exp over the workgroup
  float mw = wave_max(m);
  float sw = wave_sum(m == -INFINITY ? 0.f : s * __expf(m - mw));
  if (lane == 0) { s_red[0][wid] = mw; s_red[1][wid] = sw; }
#pragma unroll
  for (int c = 0; c < KMAX; ++c) { s_v[tid * KMAX + c] = lv[c]; s_i[tid * KMAX + c] = li[c]; }
  __syncthreads();
  float M = s_red[0][0];
  for (int w = 1; w < TOPK_THREADS / 64; ++w) M = fmaxf(M, s_red[0][w]);
  float S = 0.f;
  for (int w = 0; w < TOPK_THREADS / 64; ++w) S += s_red[1][w] * __expf(s_red[0][w] - M);
  const float logS = logf(S);
  const int beam = r % k;
  __syncthreads();  // s_red is reused below
  // K2 rounds of a workgroup argmax over the heads of the per-thread sorted lists
  int h = 0;
  for (int n = 0; n < K2; ++n) {
    float v = h < KMAX ? s_v[tid * KMAX + h] : -INFINITY;
    int i = h < KMAX ? s_i[tid * KMAX + h] : INT_MAX;
    wave_argmax(v, i);
    if (lane == 0) { s_red[n & 1][wid] = v; s_redi[n & 1][wid] = i; }
    __syncthreads();
    float bv = s_red[n & 1][0];
    int bi = s_redi[n & 1][0];
    for (int w = 1; w < TOPK_THREADS / 64; ++w)
      if (beam_better(s_red[n & 1][w], s_redi[n & 1][w], bv, bi)) { bv = s_red[n & 1][w]; bi = s_redi[n & 1][w]; }
    if (h < KMAX && s_i[tid * KMAX + h] == bi) ++h;  // indices are unique within a row: exactly one thread advances
    if (tid == 0) {
      const long o = (long)r * K2 + n;
      row_score[o] = NORMED ? bv : ((bv - M) - logS) + rs;  // log_softmax (x - max - log sum exp), then + running score
      row_idx[o] = bi == INT_MAX ? INT_MAX : beam * V + bi;
    }
  }
}

// one wave per sample: merge the k sorted row lists into the sample's K2 best
__global__ __launch_bounds__(64) void beam_topk_merge_kernel(const float* __restrict__ row_score, const int* __restrict__ row_idx, int k,
                                                             int K2, float* __restrict__ out_score, int* __restrict__ out_idx) {
  const int b = blockIdx.x, lane = threadIdx.x;
  int h = 0;
  const long base = ((long)b * k + lane) * K2;
  for (int n = 0; n < K2; ++n) {
    float v = -INFINITY;
    int i = INT_MAX;
    if (lane < k && h < K2) { v = row_score[base + h]; i = row_idx[base + h]; }
    float bv = v;
    int bi = i;
    wave_argmax(bv, bi);
    if (lane < k && h < K2 && i == bi) ++h;
    if (lane == 0) { out_score[(long)b * K2 + n] = bv; out_idx[(long)b * K2 + n] = bi; }
  }
}

// one wave per sample (B workgroups of 64); k <= 16 so the 2k candidates and the 3k merged pool entries fit the wave
__global__ __launch_bounds__(64) void beam_update_kernel(klab_beam_update_args a, int c) {
  const int b = blockIdx.x, lane = threadIdx.x, k = a.k, K2 = 2 * k, Lm = a.max_length;
  __shared__ float s_rl[32], s_ms[48], s_rs[16];
  __shared__ int s_cbeam[32], s_ctok[32], s_hit[32], s_mflag[48], s_mlen[48], s_src[16], s_par[16], s_tok[16];
  __shared__ int s_full;
  const long rb = (long)b * k;  // first row of this sample
  const float NEG = -1.0e9f;
  if (lane == 0) s_full = 1;
  __syncthreads();
  float sc = 0.f;
  int hit = 0, did = 0;
  if (lane < K2) {
    sc = a.cand_score[(long)b * K2 + lane];
    const int idx = a.cand_idx[(long)b * K2 + lane];
    const int beam = idx / a.V, tok = idx % a.V;
    hit = (tok == a.eos_id) || (c + 1 >= Lm);
    did = hit && lane < k;
    s_cbeam[lane] = beam; s_ctok[lane] = tok; s_hit[lane] = hit;
    s_rl[lane] = sc + (hit ? NEG : -0.0f);  // topk_log_probs + hits * -1e9
  }
  if (lane < k) {
    s_ms[lane] = a.fin_score[rb + lane];
    s_mflag[lane] = a.fin_flag[rb + lane];
    s_mlen[lane] = a.fin_len[rb + lane];
    if (!s_mflag[lane]) atomicAnd(&s_full, 0);
  }
  __syncthreads();
  const int unsat = a.unsat[b];
  const int full = s_full && a.early_stopping == 1;
  // running beams: the k best of topk_log_probs with the hits masked
  if (lane < K2) {
    const float rl = s_rl[lane];
    int rank = 0;
    for (int q = 0; q < K2; ++q) rank += beam_better(s_rl[q], q, rl, lane);
    if (rank < k) { s_par[rank] = s_cbeam[lane]; s_tok[rank] = s_ctok[lane]; s_rs[rank] = rl; }
    // finished candidates: length penalty, then the three -1e9 masks in HF's order
    float fs = sc / (float)pow((double)c, (double)a.length_penalty);
    fs += full ? NEG : -0.0f;
    fs += unsat ? -0.0f : NEG;
    fs += did ? -0.0f : NEG;
    s_ms[k + lane] = fs; s_mflag[k + lane] = did; s_mlen[k + lane] = c;
  }
  __syncthreads();
  // finished pool: the k best of [pool, candidates]
  if (lane < 3 * k) {
    const float v = s_ms[lane];
    int rank = 0;
    for (int q = 0; q < 3 * k; ++q) rank += beam_better(s_ms[q], q, v, lane);
    if (rank < k) s_src[rank] = lane;
  }
  __syncthreads();
  float nscore = 0.f;
  int nflag = 1;
  if (lane < k) {
    const int src = s_src[lane];
    nscore = s_ms[src]; nflag = s_mflag[src];
    a.fin_score[rb + lane] = nscore;
    a.fin_flag[rb + lane] = nflag;
    a.fin_len[rb + lane] = s_mlen[src];
    a.run_score[rb + lane] = s_rs[lane];
    a.prev_tokens[rb + lane] = s_tok[lane];
    a.parent[rb + lane] = (int)rb + s_par[lane];
  }
  // sequences (ping-pong buffers: *_in of the previous step, *_out of this one) and the key-slot table
  for (int j = 0; j < k; ++j) {
    const int src = s_src[j];
    long long* fo = a.fin_seq_out + (rb + j) * Lm;
    const long long* fi = src < k ? a.fin_seq_in + (rb + src) * Lm : a.run_seq_in + (rb + s_cbeam[src - k]) * Lm;
    const int ftok = src < k ? 0 : s_ctok[src - k];
    const long long* ri = a.run_seq_in + (rb + s_par[j]) * Lm;
    long long* ro = a.run_seq_out + (rb + j) * Lm;
    for (int p = lane; p < Lm; p += 64) {
      fo[p] = (src >= k && p == c) ? (long long)ftok : fi[p];
      ro[p] = p == c ? (long long)s_tok[j] : ri[p];
      if (a.slot_in && p <= c) a.slot_out[(rb + j) * Lm + p] = p == c ? (int)(rb + j) : a.slot_in[(rb + s_par[j]) * Lm + p];
    }
  }
  // early-stop heuristic (cur_len + 1 - decoder_prompt_len == c) and the stop bits
  if (lane < 64) {
    float mn = lane < k ? nscore : INFINITY;
    mn = -wave_max(-mn);
    const int bhl = (a.early_stopping == 2 && a.length_penalty > 0.f) ? Lm - 1 : c;
    const float best = s_rs[0] / (float)pow((double)bhl, (double)a.length_penalty);
    const int imp = lane < k && best > (nflag ? mn : NEG);
    const int nunsat = unsat && __any(imp);
    const int open = __any(lane < k && !nflag);
    const int cont = __any(lane < K2 && !s_hit[lane < K2 ? lane : 0]);
    if (lane == 0) {
      a.unsat[b] = nunsat;
      atomicOr(a.stop_word + c, (nunsat ? 1 : 0) | (open ? 2 : 0) | (cont ? 4 : 0));
    }
  }
}

// state before HF's first step: running scores 0 / -1e9 (beam 0 / the others), an empty finished pool (-1e9, unfinished),
// every sequence = start token then fill, key slot of position 0 = the row itself, stop words cleared
__global__ __launch_bounds__(64) void beam_init_kernel(klab_beam_update_args a, int start_id, int fill_id) {
  const int r = blockIdx.x, lane = threadIdx.x, Lm = a.max_length;
  long long* rs = const_cast<long long*>(a.run_seq_in) + (long)r * Lm;
  long long* fs = const_cast<long long*>(a.fin_seq_in) + (long)r * Lm;
  for (int p = lane; p < Lm; p += 64) {
    rs[p] = p == 0 ? start_id : fill_id;
    fs[p] = p == 0 ? start_id : fill_id;
    if (r == 0) a.stop_word[p] = 0;
  }
  if (lane == 0) {
    if (a.slot_in) const_cast<int*>(a.slot_in)[(long)r * Lm] = r;
    a.run_score[r] = (r % a.k) == 0 ? 0.f : -1.0e9f;
    a.fin_score[r] = -1.0e9f; a.fin_flag[r] = 0; a.fin_len[r] = 0;
    if ((r % a.k) == 0) a.unsat[r / a.k] = 1;
  }
}

template <typename T>
__global__ void copy_rows_kernel(const T* __restrict__ src, long src_ld, int src_div, T* __restrict__ dst, long dst_ld, int cols) {
  const int r = blockIdx.x;
  const T* s = src + (long)(r / src_div) * src_ld;
  T* d = dst + (long)r * dst_ld;
  for (int c = threadIdx.x; c < cols; c += blockDim.x) d[c] = s[c];
}

template <typename T, int KMAX, bool NORMED>
static void launch_rows(const void* logits, long ld, int row_div, const float* rs, int B, int k, int V, float* rsc, int* ri, hipStream_t s) {
  hipLaunchKernelGGL((beam_topk_rows_kernel<T, KMAX, NORMED>), dim3(B * k), dim3(topk_threads<KMAX>()), 0, s, (const T*)logits, ld, row_div, rs, k, V, 2 * k,
                     rsc, ri);
}

template <typename T, bool NORMED = false>
static int topk_dispatch(const void* logits, long ld, int row_div, const float* rs, int B, int k, int V, float* rsc, int* ri, hipStream_t s) {
  const int K2 = 2 * k;
  if (K2 <= 2) launch_rows<T, 2, NORMED>(logits, ld, row_div, rs, B, k, V, rsc, ri, s);
  else if (K2 <= 4) launch_rows<T, 4, NORMED>(logits, ld, row_div, rs, B, k, V, rsc, ri, s);
  else if (K2 <= 8) launch_rows<T, 8, NORMED>(logits, ld, row_div, rs, B, k, V, rsc, ri, s);
  else if (K2 <= 16) launch_rows<T, 16, NORMED>(logits, ld, row_div, rs, B, k, V, rsc, ri, s);
  else launch_rows<T, 32, NORMED>(logits, ld, row_div, rs, B, k, V, rsc, ri, s);
  KLAB_LAUNCH_CHECK();
  return KLAB_OK;
}

}  // namespace klab

extern "C" int klab_beam_topk(int dtype, const void* logits, long ld, int row_div, const float* run_score, int B, int k, int V,
                              float* row_score, int* row_idx, float* out_score, int* out_idx, void* stream) {
  using namespace klab;
  if (!logits || !run_score || !row_score || !row_idx || !out_score || !out_idx || B <= 0 || k < 1 || k > 16 || row_div < 1 ||
      V < 2 * k || ld < V)
    return KLAB_ERR_BADARG;
  hipStream_t s = (hipStream_t)stream;
  int rc;
  if (dtype == KLAB_BF16) rc = topk_dispatch<bf16_t>(logits, ld, row_div, run_score, B, k, V, row_score, row_idx, s);
  else if (dtype == KLAB_F32) rc = topk_dispatch<float>(logits, ld, row_div, run_score, B, k, V, row_score, row_idx, s);
  else return KLAB_ERR_BADARG;
  if (rc) return rc;
  hipLaunchKernelGGL(beam_topk_merge_kernel, dim3(B), dim3(64), 0, s, row_score, row_idx, k, 2 * k, out_score, out_idx);
  KLAB_LAUNCH_CHECK();
  return KLAB_OK;
}

extern "C" int klab_beam_topk_scores(const float* scores, long ld, int row_div, const float* run_score, int B, int k, int V,
                                     float* row_score, int* row_idx, float* out_score, int* out_idx, void* stream) {
  using namespace klab;
  if (!scores || !run_score || !row_score || !row_idx || !out_score || !out_idx || B <= 0 || k < 1 || k > 16 || row_div < 1 ||
      V < 2 * k || ld < V)
    return KLAB_ERR_BADARG;
  hipStream_t s = (hipStream_t)stream;
  const int rc = topk_dispatch<float, true>(scores, ld, row_div, run_score, B, k, V, row_score, row_idx, s);
  if (rc) return rc;
  hipLaunchKernelGGL(beam_topk_merge_kernel, dim3(B), dim3(64), 0, s, row_score, row_idx, k, 2 * k, out_score, out_idx);
  KLAB_LAUNCH_CHECK();
  return KLAB_OK;
}

extern "C" int klab_beam_update(const klab_beam_update_args* a, int cur_len, void* stream) {
  using namespace klab;
  if (!a || a->B <= 0 || a->k < 1 || a->k > 16 || a->V < 2 * a->k || cur_len < 1 || cur_len >= a->max_length || !a->cand_score ||
      !a->cand_idx || !a->run_seq_in || !a->run_seq_out || !a->run_score || !a->fin_seq_in || !a->fin_seq_out || !a->fin_score ||
      !a->fin_flag || !a->fin_len || !a->unsat || !a->prev_tokens || !a->parent || !a->stop_word || (!a->slot_in != !a->slot_out) ||
      a->early_stopping < 0 || a->early_stopping > 2)
    return KLAB_ERR_BADARG;
  hipLaunchKernelGGL(beam_update_kernel, dim3(a->B), dim3(64), 0, (hipStream_t)stream, *a, cur_len);
  KLAB_LAUNCH_CHECK();
  return KLAB_OK;
}

extern "C" int klab_beam_init(const klab_beam_update_args* a, int start_id, int fill_id, void* stream) {
  using namespace klab;
  if (!a || a->B <= 0 || a->k < 1 || a->k > 16 || a->max_length < 2 || !a->run_seq_in || !a->fin_seq_in || !a->run_score ||
      !a->fin_score || !a->fin_flag || !a->fin_len || !a->unsat || !a->stop_word)
    return KLAB_ERR_BADARG;
  hipLaunchKernelGGL(beam_init_kernel, dim3(a->B * a->k), dim3(64), 0, (hipStream_t)stream, *a, start_id, fill_id);
  KLAB_LAUNCH_CHECK();
  return KLAB_OK;
}

extern "C" int klab_beam_copy_rows(int elem_bytes, const void* src, long src_ld, int src_div, void* dst, long dst_ld, int rows, int cols,
                                   void* stream) {
  using namespace klab;
  if (!src || !dst || rows <= 0 || cols <= 0 || src_div < 1) return KLAB_ERR_BADARG;
  hipStream_t s = (hipStream_t)stream;
  if (elem_bytes == 2)
    hipLaunchKernelGGL(copy_rows_kernel<uint16_t>, dim3(rows), dim3(256), 0, s, (const uint16_t*)src, src_ld, src_div, (uint16_t*)dst, dst_ld, cols);
  else if (elem_bytes == 4)
    hipLaunchKernelGGL(copy_rows_kernel<uint32_t>, dim3(rows), dim3(256), 0, s, (const uint32_t*)src, src_ld, src_div, (uint32_t*)dst, dst_ld, cols);
  else if (elem_bytes == 8)
    hipLaunchKernelGGL(copy_rows_kernel<uint64_t>, dim3(rows), dim3(256), 0, s, (const uint64_t*)src, src_ld, src_div, (uint64_t*)dst, dst_ld, cols);
  else return KLAB_ERR_BADARG;
  KLAB_LAUNCH_CHECK();
  return KLAB_OK;
}
