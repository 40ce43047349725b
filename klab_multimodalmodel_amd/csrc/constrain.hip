// Trie-constrained decoding on the device (HF's PrefixConstrainedLogitsProcessor / `prefix_allowed_tokens_fn` without the host
// callback): every row stands on a node of a token trie in CSR form (child_off / child_tok ascending within a node / child_node;
// klab_multimodalmodel_amd/constrain.py builds it) and may only choose one of the node's children.
//
//   klab_constrain_rows : one 1024-thread workgroup per row, the row in registers as in klab_logits_process_rows (row_regs.h: thread
//                         t owns the 32 tokens of bit word t of an LDS bitmap over the vocabulary, V <= 32768).
//     1. advance: wave 0 moves the row's node over the token chosen last -- node_out[r] = child(node_in[parent ? parent[r] : r],
//        last_tok[r]), or the root of the row's image at the first position.  The child search is 64-ary over the ascending
//        child_tok: each round the 64 lanes probe 64 evenly spaced edges at once and one ballot narrows the range 64-fold, so a node
//        of 32768 children costs three rounds of independent loads, not fifteen dependent ones.  -1 = off the trie; it stays -1.
//     2. scores = fp32 logits, or their log_softmax over the WHOLE row (beam search; row_log_softmax, the reduction of
//        klab_logits_process_rows, so the allowed entries carry the bits beam search scores without a constraint).
//     3. the allowed set goes to the bitmap: one thread per edge of the node sets its token's bit; a node without children and the
//        state -1 allow exactly eos_id (the row ends).  The bitmap makes the result independent of the order of the LDS atomics.
//     4. every thread writes its own 32 scores, -inf where its word has no bit.  It read exactly these 32 before, so `out` may be the
//        f32 input itself.
#include <math.h>

#include "common.h"
#include "klab_mm.h"
#include "row_regs.h"

namespace klab {

// wave-cooperative: the index of edge `tok` among child_tok[lo, hi) (ascending), -1 without one; all 64 lanes call it with the same
// arguments and get the same answer
__device__ __forceinline__ int trie_find_edge(const int* __restrict__ child_tok, int lo, int hi, int tok, int lane) {
  while (hi - lo > 64) {
    const int step = (hi - lo + 63) >> 6;  // lane l probes the first edge of its slice [lo + l*step, lo + (l+1)*step)
    const int i = lo + lane * step;
    const bool le = i < hi && child_tok[i] <= tok;  // ascending: the lanes that hold are a prefix of the wave
    const int cnt = __popcll(__ballot(le));
    if (cnt == 0) return -1;  // below the node's first edge
    lo += (cnt - 1) * step;
    hi = min(hi, lo + step);
  }
  const int i = lo + lane;
  const unsigned long long hit = __ballot(i < hi && child_tok[i] == tok);
  return hit ? lo + __ffsll((long long)hit) - 1 : -1;
}

__global__ __launch_bounds__(PROC_THREADS) void constrain_rows_kernel(klab_constrain_args a) {
  __shared__ uint32_t s_allow[PROC_THREADS];
  __shared__ float s_f[2][PROC_WAVES];
  __shared__ int s_node;
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int V = a.V, j0 = tid * PROC_NPT;
  const int nv = max(0, min(PROC_NPT, V - j0));
  s_allow[tid] = 0u;
  float v[PROC_NPT];  // (loaded first: wave 0's chain of dependent table reads below then runs under the row's loads)
  row_load(v, a.dtype, a.logits, (long)(r / a.row_div) * a.ld + j0, nv);
  // 1. the row's node (every index read from memory is checked against the table sizes before it is used)
  if (tid < 64) {
    int node;
    if (a.first) {
      node = a.root[r / a.root_div];
    } else {
      node = a.node_in[a.parent ? a.parent[r] : r];
      const long long t = a.last_tok[r];
      if (node >= 0 && node < a.n_nodes && t >= 0 && t < V) {
        const int lo = max(0, min(a.child_off[node], a.n_edges)), hi = max(lo, min(a.child_off[node + 1], a.n_edges));
        const int e = trie_find_edge(a.child_tok, lo, hi, (int)t, lane);
        node = e >= 0 ? a.child_node[e] : -1;
      } else {
        node = -1;
      }
    }
    if (node < 0 || node >= a.n_nodes) node = -1;
    if (tid == 0) { s_node = node; a.node_out[r] = node; }
  }
  // 2. scores
  if (a.log_softmax) row_log_softmax(v, nv, s_f);
  __syncthreads();  // the node and the cleared bitmap
  // 3. the allowed set
  const int node = s_node;
  int lo = 0, hi = 0;
  if (node >= 0) {
    lo = max(0, min(a.child_off[node], a.n_edges));
    hi = max(lo, min(a.child_off[node + 1], a.n_edges));
  }
  if (hi == lo) {
    if (tid == 0 && a.eos_id >= 0 && a.eos_id < V) atomicOr(&s_allow[a.eos_id >> 5], 1u << (a.eos_id & 31));
  } else {
    for (int e = lo + tid; e < hi; e += PROC_THREADS) {
      const int t = a.child_tok[e];
      if (t >= 0 && t < V) atomicOr(&s_allow[t >> 5], 1u << (t & 31));
    }
  }
  __syncthreads();
  // 4. this thread's word
  const uint32_t am = s_allow[tid];
#pragma unroll
  for (int c = 0; c < PROC_NPT; ++c)
    if (!((am >> c) & 1u)) v[c] = -INFINITY;
  row_store(v, a.out + (long)r * a.ld_out + j0, nv);
}

}  // namespace klab

extern "C" int klab_sizeof_constrain_args(void) { return (int)sizeof(klab_constrain_args); }

extern "C" int klab_constrain_rows(const klab_constrain_args* a, void* stream) {
  using namespace klab;
  if (!a || !a->logits || !a->out || !a->node_out || !a->child_off || a->rows <= 0 || a->V < 1 || a->row_div < 1 || a->ld < a->V ||
      a->ld_out < a->V || a->n_nodes < 1 || a->n_edges < 0 || (a->n_edges > 0 && (!a->child_tok || !a->child_node)) ||
      a->n_edges > a->n_nodes - 1 ||  // (every node has at most one edge into it, a root none)
      (a->first ? !a->root || a->root_div < 1 : !a->node_in || !a->last_tok || (a->parent && a->node_in == a->node_out)))
    return KLAB_ERR_BADARG;
  if (a->V > PROC_THREADS * PROC_NPT) return KLAB_ERR_UNSUPPORTED;
  if (a->dtype != KLAB_F32 && a->dtype != KLAB_BF16) return KLAB_ERR_BADARG;
  hipLaunchKernelGGL(constrain_rows_kernel, dim3(a->rows), dim3(PROC_THREADS), 0, (hipStream_t)stream, *a);
  KLAB_LAUNCH_CHECK();
  return KLAB_OK;
}
