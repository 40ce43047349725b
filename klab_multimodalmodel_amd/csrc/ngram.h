// The n-gram conventions the caption kernels share (scst.hip: CIDEr-D rewards; metrics.hip: BLEU / ROUGE-L statistics).
// A sequence's units are its tokens through the first EOS (the EOS itself when count_eos); an id < 0 or >= 0xFFFF ends it.  At most
// 64 units, so the n-grams of one order fit one wave64: lane i owns the n-gram that starts at unit i.  Its key is exact,
// t0 | t1 << 16 | t2 << 32 | t3 << 48 with 0xFFFF in the absent positions -- ids only ever form keys, never addresses -- so the
// all-ones key cannot occur and marks an empty slot.
#pragma once
#include "common.h"

namespace klab {

constexpr int SC_UNITS = 64;   // units of a sequence = lanes of a wave
constexpr int SC_MAX_R = 16;
constexpr int SC_ORDERS = 4;
constexpr unsigned long long SC_EMPTY = ~0ull;

// lane i holds token i of a row of `width` tokens (anything beyond `width` is not looked at); returns the number of units and
// leaves 0xFFFF in the lanes that hold none
__device__ __forceinline__ int seq_units(long long& tok, int lane, int width, int eos, int count_eos) {
  const bool in = lane < width;
  const bool bad = in && (tok < 0 || tok >= 0xFFFF);
  const bool end = in && !bad && tok == eos;
  const unsigned long long stops = __ballot(bad || end);
  int len = width;
  if (stops) {
    const int p = __ffsll((long long)stops) - 1;
    len = p + (((__ballot(end) >> p) & 1ull) && count_eos ? 1 : 0);
  }
  if (lane >= len) tok = 0xFFFF;
  return len;
}

// the n-gram of order n that starts at this lane's unit: key, number of occurrences in the sequence and whether this lane is the
// first of them.  valid: the n-gram lies inside the sequence
struct Gram {
  unsigned long long key;
  int count;
  bool valid, first;
};
__device__ __forceinline__ Gram wave_gram(long long tok, int lane, int len, int n) {
  Gram g;
  g.key = (unsigned long long)tok & 0xFFFFull;
#pragma unroll
  for (int k = 1; k < SC_ORDERS; ++k) {
    const unsigned long long t = (unsigned long long)__shfl_down(tok, k, 64) & 0xFFFFull;  // (lanes it cannot reach are not valid)
    g.key |= (k < n ? t : 0xFFFFull) << (16 * k);
  }
  const int grams = len - n + 1;
  g.valid = lane < grams;
  int c = 0;
  bool first = true;
  for (int k = 0; k < grams; ++k) {  // (grams is wave-uniform)
    const bool same = __shfl(g.key, k, 64) == g.key;
    c += same;
    first = first && !(same && k < lane);
  }
  g.count = c;
  g.first = g.valid && first;
  return g;
}

}  // namespace klab
