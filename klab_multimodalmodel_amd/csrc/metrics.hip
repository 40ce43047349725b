// Caption metrics on the device: the integer sufficient statistics of BLEU-1..4 and ROUGE-L of every hypothesis against its
// image's reference captions (klab_caption_stats), over units = token ids under the conventions of ngram.h.  One launch whatever
// B, n and R; no floating point, no atomics, no table outside the image's own references; every output element stored once.
//
//   stats[r][0..3]  match_n = sum over the hypothesis' distinct n-grams g of min(count_h(g), max_j count_j(g))      n = 1..4
//   stats[r][4..7]  guess_n = max(0, len_h - n + 1)
//   stats[r][8]     len_h           [9] the present reference length closest to len_h, the shorter one on a tie
//   stats[r][10]    max_j LCS(h, r_j)
//   stats[r][11,12] the (lcs_j, len_j) with the largest lcs_j / len_j by exact cross-multiplication (lowest j on a tie; references
//                   without units skipped; (0, 0) when there is none)
//   stats[r][13]    the number of present references          [14, 15] 0
//   an image without present references: a row of zeros
//
// One workgroup per image.  Its eight waves stage each reference once as ONE 64-bit word per unit: the order-4 key of the n-gram
// that starts there, 0xFFFF where the sequence has ended.  The key of order n is that word with the positions >= n filled with
// ones, so one LDS word serves all four orders, and a word that equals a hypothesis n-gram's key is an n-gram INSIDE the reference
// (a hypothesis key holds units, which are < 0xFFFF, in its first n positions).  The waves then stride over the image's hypotheses:
// lane i owns the n-gram that starts at unit i and counts it in every reference (a broadcast LDS read per reference unit).
//
// LCS: the bit-parallel recurrence (Crochemore et al. / Hyyro) on one 64-bit word per pair -- lane i holds reference unit i; per
// hypothesis unit t, M = ballot(ref_i == t), U = V & M, V = (V + U) | (V & ~M); LCS = popcount(~V & mask).  Wave-uniform throughout.
#include "common.h"
#include "klab_mm.h"
#include "ngram.h"

namespace klab {
namespace {

constexpr int MT_WAVES = 8;  // per workgroup, as the rewards kernel: five references and five hypotheses cost one sequence per wave
constexpr int MT_STATS = 16;

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ones in the 16-bit positions >= n of a key
__device__ __forceinline__ constexpr unsigned long long absent_positions(int n) { return n >= SC_ORDERS ? 0ull : ~0ull << (16 * n); }

__global__ __launch_bounds__(64 * MT_WAVES) void caption_stats_kernel(const long long* __restrict__ hyp, int n_h, int L,
                                                                      const long long* __restrict__ refs, int R, int Lr, int eos,
                                                                      int count_eos, int* __restrict__ stats) {
  __shared__ unsigned long long r_word[SC_MAX_R][SC_UNITS];
  __shared__ int r_len[SC_MAX_R];  // -1: the reference is absent
  const int img = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

  for (int j = wave; j < R; j += MT_WAVES) {
    const long long* row = refs + ((long)img * R + j) * Lr;
    long long tok = lane < Lr ? row[lane] : -1;
    const bool present = __shfl(tok, 0, 64) >= 0;
    const int len = seq_units(tok, lane, Lr, eos, count_eos);  // (tok is 0xFFFF from the end on)
    unsigned long long w = (unsigned long long)tok;
#pragma unroll
    for (int k = 1; k < SC_ORDERS; ++k) {
      const unsigned long long t = (unsigned long long)__shfl_down(tok, k, 64);
      w |= (lane + k < SC_UNITS ? t : 0xFFFFull) << (16 * k);
    }
    r_word[j][lane] = w;
    if (lane == 0) r_len[j] = present ? len : -1;
  }
  __syncthreads();

  int present = 0;
  for (int j = 0; j < R; ++j) present += r_len[j] >= 0;
  for (int h = wave; h < n_h; h += MT_WAVES) {
    const long r = (long)img * n_h + h;
    const long long* row = hyp + r * L + 1;  // column 0 is the start token
    long long tok = lane < L - 1 ? row[lane] : -1;
    const int len = seq_units(tok, lane, L - 1, eos, count_eos);
    int v[MT_STATS];
#pragma unroll
    for (int k = 0; k < MT_STATS; ++k) v[k] = 0;
    if (present > 0) {
      // clipped matches
      Gram g[SC_ORDERS];
      int clip[SC_ORDERS];
#pragma unroll
      for (int n = 0; n < SC_ORDERS; ++n) {
        g[n] = wave_gram(tok, lane, len, n + 1);
        clip[n] = 0;
      }
      for (int j = 0; j < R; ++j) {
        const int lj = r_len[j];
        if (lj <= 0) continue;
        int c[SC_ORDERS] = {0, 0, 0, 0};
        for (int m = 0; m < lj; ++m) {
          const unsigned long long w = r_word[j][m];
#pragma unroll
          for (int n = 0; n < SC_ORDERS; ++n) c[n] += (w | absent_positions(n + 1)) == g[n].key;
        }
#pragma unroll
        for (int n = 0; n < SC_ORDERS; ++n) clip[n] = max(clip[n], c[n]);
      }
#pragma unroll
      for (int n = 0; n < SC_ORDERS; ++n) {
        v[n] = wave_sum_int(g[n].first ? min(g[n].count, clip[n]) : 0);
        v[4 + n] = max(0, len - n);
      }
      v[8] = len;
      // closest reference length, LCS
      int close = -1, lcs_max = 0, best_lcs = 0, best_len = 0;
      for (int j = 0; j < R; ++j) {
        const int lj = r_len[j];
        if (lj < 0) continue;
        if (close < 0 || abs(lj - len) < abs(close - len) || (abs(lj - len) == abs(close - len) && lj < close)) close = lj;
        if (lj == 0) continue;
        const unsigned long long unit = r_word[j][lane] & 0xFFFFull;  // 0xFFFF from the reference's end on: equals no unit
        const unsigned long long mask = lj >= 64 ? ~0ull : (1ull << lj) - 1ull;
        unsigned long long V = ~0ull;
        for (int t = 0; t < len; ++t) {
          const unsigned long long ht = (unsigned long long)__shfl(tok, t, 64);
          const unsigned long long M = __ballot(unit == ht) & mask;
          const unsigned long long U = V & M;
          V = (V + U) | (V & ~M);
        }
        const int lcs = __popcll(~V & mask);
        lcs_max = max(lcs_max, lcs);
        if (best_len == 0 || lcs * best_len > best_lcs * lj) {
          best_lcs = lcs;
          best_len = lj;
        }
      }
      v[9] = close;
      v[10] = lcs_max;
      v[11] = best_lcs;
      v[12] = best_len;
      v[13] = present;
    }
    int mine = 0;
#pragma unroll
    for (int k = 0; k < MT_STATS; ++k) mine = lane == k ? v[k] : mine;
    if (lane < MT_STATS) stats[r * MT_STATS + lane] = mine;
  }
}

}  // namespace
}  // namespace klab

using namespace klab;

extern "C" int klab_caption_stats(const long long* hyp, int rows, int n_h, int L, const long long* refs, int R, int Lr, int eos,
                                  int count_eos, int* stats, void* stream) {
  if (!hyp || !refs || !stats || rows <= 0 || n_h <= 0 || rows % n_h || L < 1 || Lr < 1 || eos < 0 || eos >= 0xFFFF) return KLAB_ERR_BADARG;
  if (L > SC_UNITS + 1 || Lr > SC_UNITS || R < 1 || R > SC_MAX_R) return KLAB_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(caption_stats_kernel, dim3(rows / n_h), dim3(64 * MT_WAVES), 0, (hipStream_t)stream, hyp, n_h, L, refs, R, Lr, eos,
                     count_eos ? 1 : 0, stats);
  KLAB_LAUNCH_CHECK();
  return KLAB_OK;
}
