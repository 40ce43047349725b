// Self-critical sequence training on the device: the CIDEr-D reward of sampled captions against each image's reference captions
// (klab_ciderd_rewards) and the labels, per-token weights and advantages of the training forward that follows (klab_scst_targets).
// One launch each, whatever B, n and R; no host read, no floating-point atomics, fixed summation order.
//
// CIDEr-D over units = token ids.  A sequence's units are its tokens through the first EOS (the EOS itself when count_eos); an id
// < 0 or >= 0xFFFF ends it.  At most 64 units, so the n-grams of one order fit one wave64: lane i owns the n-gram that starts at
// unit i.  Its key is exact, t0 | t1 << 16 | t2 << 32 | t3 << 48 with 0xFFFF in the absent positions -- ids only ever form keys,
// never addresses -- so the all-ones key cannot occur and marks an empty slot, in the idf table and in the staged references.
//
//   vec(g)  = count(g) idf(g)           idf from the table, log_n for an n-gram it does not hold
//   sim_j   = sum_{g in hyp} min(vec_h(g), vec_j(g)) vec_j(g) / (norm_h norm_j)  (divided when both norms are non-zero)
//             times exp(-(len_h - len_j)^2 / (2 sigma^2))
//   reward  = 10 mean_{n = 1..4} mean_{j present} sim_j
//
// One workgroup per image: its eight waves stage the references once -- per order and reference the keys of the DISTINCT n-grams
// (the lane of an n-gram's first occurrence; the others store the empty key) and their weighted counts -- then stride over the
// image's hypotheses, so a reference is processed once, not once per hypothesis.
#include <math.h>

#include "common.h"
#include "klab_mm.h"
#include "ngram.h"

namespace klab {
namespace {

constexpr unsigned long long SC_GOLDEN = 0x9E3779B97F4A7C15ull;

struct IdfTable {
  const unsigned long long* keys;
  const float* idf;
  unsigned long long mask;  // cap - 1
  int shift;                // 64 - log2 cap
  float log_n;
};

// linear probing from `slot`, wrapping; bounded by the capacity (a full table cannot spin)
__device__ __forceinline__ float idf_probe(const IdfTable& t, unsigned long long key, unsigned long long slot) {
  for (unsigned long long p = 0; p <= t.mask; ++p) {
    const unsigned long long k = t.keys[slot];
    if (k == key) return t.idf[slot];
    if (k == SC_EMPTY) break;
    slot = (slot + 1) & t.mask;
  }
  return t.log_n;
}

// count * idf of the lane's n-gram of each order (0 unless the lane is the n-gram's first occurrence).  A probe is two dependent
// loads and a sequence has four of them: the home slots' keys AND values of all four orders are loaded first (eight independent
// loads; the slot is masked, so the speculative value load is in bounds), and only a collision walks on -- at a load factor of
// at most 1/2 most n-grams sit in their home slot.
__device__ __forceinline__ void weigh(const IdfTable& t, const Gram (&g)[SC_ORDERS], float (&v)[SC_ORDERS]) {
  unsigned long long slot[SC_ORDERS], k[SC_ORDERS];
  float w[SC_ORDERS];
#pragma unroll
  for (int n = 0; n < SC_ORDERS; ++n) {
    slot[n] = (g[n].key * SC_GOLDEN) >> t.shift;
    k[n] = t.keys[slot[n]];
    w[n] = t.idf[slot[n]];
  }
#pragma unroll
  for (int n = 0; n < SC_ORDERS; ++n) {
    v[n] = 0.f;
    if (g[n].first) {
      if (k[n] != g[n].key) w[n] = k[n] == SC_EMPTY ? t.log_n : idf_probe(t, g[n].key, (slot[n] + 1) & t.mask);
      v[n] = (float)g[n].count * w[n];
    }
  }
}

constexpr int SC_WAVES = 8;  // per workgroup: five references and five hypotheses then cost one sequence per wave, not two

__global__ __launch_bounds__(64 * SC_WAVES) void ciderd_rewards_kernel(const long long* __restrict__ hyp, int n_h, int L,
                                                             const long long* __restrict__ refs, int R, int Lr, IdfTable tab, float sigma,
                                                             int eos, int count_eos, float* __restrict__ out) {
  __shared__ unsigned long long r_key[SC_ORDERS][SC_MAX_R][SC_UNITS];
  __shared__ float r_vec[SC_ORDERS][SC_MAX_R][SC_UNITS];
  __shared__ float r_norm[SC_ORDERS][SC_MAX_R];
  __shared__ int r_len[SC_MAX_R];  // -1: the reference is absent
  const int img = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

  for (int j = wave; j < R; j += SC_WAVES) {
    const long long* row = refs + ((long)img * R + j) * Lr;
    long long tok = lane < Lr ? row[lane] : -1;
    const bool present = __shfl(tok, 0, 64) >= 0;
    const int len = seq_units(tok, lane, Lr, eos, count_eos);
    if (lane == 0) r_len[j] = present ? len : -1;
    Gram g[SC_ORDERS];
    float v[SC_ORDERS];
#pragma unroll
    for (int n = 1; n <= SC_ORDERS; ++n) g[n - 1] = wave_gram(tok, lane, len, n);
    weigh(tab, g, v);
#pragma unroll
    for (int n = 0; n < SC_ORDERS; ++n) {
      r_key[n][j][lane] = g[n].first ? g[n].key : SC_EMPTY;
      r_vec[n][j][lane] = v[n];
      const float nn = wave_sum(v[n] * v[n]);
      if (lane == 0) r_norm[n][j] = sqrtf(nn);
    }
  }
  __syncthreads();

  int present = 0;
  for (int j = 0; j < R; ++j) present += r_len[j] >= 0;
  for (int h = wave; h < n_h; h += SC_WAVES) {
    const long r = (long)img * n_h + h;
    const long long* row = hyp + r * L + 1;  // column 0 is the start token
    long long tok = lane < L - 1 ? row[lane] : -1;
    const int len = seq_units(tok, lane, L - 1, eos, count_eos);
    float total = 0.f;
    if (present > 0 && len > 0) {
      Gram gs[SC_ORDERS];
      float vs[SC_ORDERS];
#pragma unroll
      for (int n = 1; n <= SC_ORDERS; ++n) gs[n - 1] = wave_gram(tok, lane, len, n);
      weigh(tab, gs, vs);
#pragma unroll
      for (int n = 1; n <= SC_ORDERS; ++n) {
        const Gram g = gs[n - 1];
        const float vh = vs[n - 1];
        const float norm_h = sqrtf(wave_sum(vh * vh));
        float score = 0.f;
        for (int j = 0; j < R; ++j) {
          const int lj = r_len[j];
          if (lj < 0) continue;
          float vj = 0.f;
          if (g.first) {
            for (int m = 0; m < lj - n + 1; ++m)
              if (r_key[n - 1][j][m] == g.key) vj = r_vec[n - 1][j][m];
          }
          float sim = wave_sum(fminf(vh, vj) * vj);
          const float norm_j = r_norm[n - 1][j];
          if (norm_h != 0.f && norm_j != 0.f) sim /= norm_h * norm_j;
          const float d = (float)(len - lj);
          sim *= expf(-(d * d) / (2.f * sigma * sigma));
          score += sim;
        }
        total += score / (float)present;
      }
    }
    if (lane == 0) out[r] = present > 0 && len > 0 ? 10.f * (total / (float)SC_ORDERS) : 0.f;
  }
}

// one wave per sequence: labels and weights of its Lt columns, its advantage
__global__ __launch_bounds__(256) void scst_targets_kernel(const long long* __restrict__ seq, int rows, int n, int L,
                                                           const float* __restrict__ rewards, const float* __restrict__ baseline, int mode,
                                                           int eos, int Lt, long long* __restrict__ labels, float* __restrict__ weights,
                                                           float* __restrict__ advantages) {
  const int lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;  // (whole waves)
  const long b = r / n;
  float adv = rewards[r];
  if (mode == 0) {
    adv -= baseline[b];
  } else if (mode == 1) {
    float others = 0.f;
    for (long k = b * n; k < (b + 1) * n; ++k)
      if (k != r) others += rewards[k];
    adv -= others / (float)(n - 1);
  }
  const long long* row = seq + r * L + 1;
  int last = L - 2;  // the last scored label column: the first EOS, or all L - 1 tokens without one
  for (int t0 = 0; t0 < L - 1; t0 += 64) {
    const int t = t0 + lane;
    const unsigned long long hit = __ballot(t < L - 1 && row[t] == eos);
    if (hit) {
      last = t0 + __ffsll((long long)hit) - 1;
      break;
    }
  }
  for (int t = lane; t < Lt; t += 64) {
    const bool scored = t <= last;
    labels[r * Lt + t] = scored ? row[t] : -100;
    weights[r * Lt + t] = scored ? adv : 0.f;
  }
  if (lane == 0) advantages[r] = adv;
}

}  // namespace
}  // namespace klab

using namespace klab;

extern "C" int klab_ciderd_rewards(const long long* hyp, int rows, int n_h, int L, const long long* refs, int R, int Lr,
                                   const unsigned long long* keys, const float* idf, long cap, float log_n, float sigma, int eos,
                                   int count_eos, float* out, void* stream) {
  if (!hyp || !refs || !keys || !idf || !out || rows <= 0 || n_h <= 0 || rows % n_h || L < 1 || Lr < 1) return KLAB_ERR_BADARG;
  if (cap < 2 || (cap & (cap - 1)) || !(sigma > 0.f) || !isfinite(sigma) || !isfinite(log_n) || eos < 0 || eos >= 0xFFFF) return KLAB_ERR_BADARG;
  if (L > SC_UNITS + 1 || Lr > SC_UNITS || R < 1 || R > SC_MAX_R) return KLAB_ERR_UNSUPPORTED;
  int lg = 0;
  while ((1L << lg) < cap) ++lg;
  const IdfTable tab{keys, idf, (unsigned long long)cap - 1, 64 - lg, log_n};
  hipLaunchKernelGGL(ciderd_rewards_kernel, dim3(rows / n_h), dim3(64 * SC_WAVES), 0, (hipStream_t)stream, hyp, n_h, L, refs, R, Lr, tab, sigma, eos,
                     count_eos ? 1 : 0, out);
  KLAB_LAUNCH_CHECK();
  return KLAB_OK;
}

extern "C" int klab_scst_targets(const long long* seq, int rows, int n, int L, const float* rewards, const float* baseline, int mode, int eos,
                                 int Lt, long long* labels, float* weights, float* advantages, void* stream) {
  if (!seq || !rewards || !labels || !weights || !advantages || rows <= 0 || n <= 0 || rows % n || L < 2 || Lt < L - 1) return KLAB_ERR_BADARG;
  if (mode < 0 || mode > 2 || (mode == 0 && !baseline) || (mode == 1 && n < 2)) return KLAB_ERR_BADARG;
  hipLaunchKernelGGL(scst_targets_kernel, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, seq, rows, n, L, rewards, baseline, mode, eos,
                     Lt, labels, weights, advantages);
  KLAB_LAUNCH_CHECK();
  return KLAB_OK;
}
