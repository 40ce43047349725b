// Head-mean cross-attention probabilities of one decode position (klab_t5_decode_attn_map, include/klab_mm.h): what HF returns as
// `cross_attentions` with output_attentions=True (HF/t5:196-213), averaged over the heads, for the single query row of each of R
// decoding rows.  A maps-only kernel beside decode_attn_kernel (attn_t5.hip), which forms the context with an online softmax and
// never holds a probability: this one reads q and K, never V, and writes no context, so asking for maps cannot change a token.
//   map[r, j] = (1 / H) * sum_h softmax_j(q_h . k_{h, j} + bias_row[h, j])        (scores unscaled, HF/t5:196-197)
// One workgroup of NW waves per (row, tile of TK keys); the waves take the heads NW at a time, head h0 + w to wave w; lanes split
// the keys as in decode_attn_kernel.  A wave scores every key of its head once: the tile's keys stay in registers, the others
// only feed the online (m, l) of the lane, merged over the wave.  The probabilities exp(s - m) / l of the tile go to the wave's LDS
// row, and the thread that owns key t adds the rows of the round to its register in wave order, i.e. in ascending h: the head sum
// is ((p_0 + p_1) + p_2) + ... in f32 for every H, no atomics, bit-reproducible; the mean is that sum times 1.0f / H (exact for a
// power-of-two H).  Key tiles beyond the first (Le > TK: not the caption shapes, 49 image + a few text tokens) repeat the (m, l)
// pass; K is then read from L2.
#include "common.h"
#include "klab_mm.h"

namespace klab {
namespace {
constexpr int MAP_NW = 4;             // waves per workgroup = heads per round
constexpr int MAP_KPL = 4;            // keys per lane in a tile
constexpr int MAP_TK = 64 * MAP_KPL;  // keys per tile = threads per workgroup: thread t owns key t of the tile

// q_h . k_j in f32, c ascending (VEC: 16-byte loads of the key row; the sum is the same expression either way)
template <typename T, int DK, bool VEC>
__device__ __forceinline__ float map_score(const float (&qv)[DK], const T* __restrict__ kr) {
  float s = 0.f;
  if constexpr (VEC) {
    using V = typename Vec16<T>::type;
    constexpr int N = Vec16<T>::N;
#pragma unroll
    for (int c = 0; c < DK; c += N) {
      const V kv = *reinterpret_cast<const V*>(kr + c);
#pragma unroll
      for (int u = 0; u < N; ++u) s += qv[c + u] * to_f32(kv[u]);
    }
  } else {
#pragma unroll
    for (int c = 0; c < DK; ++c) s += qv[c] * to_f32(kr[c]);
  }
  return s;
}

template <typename T, int DK, bool VEC>
__global__ __launch_bounds__(MAP_TK) void decode_attn_map_kernel(const T* __restrict__ q, long q_bstride, int q_div, const T* __restrict__ k,
                                                                 long kv_bstride, long ldk, int kv_group, const float* __restrict__ bias_row,
                                                                 long bias_ld, const int* __restrict__ done, float* __restrict__ map,
                                                                 long map_bstride, int H, int Lk) {
  __shared__ float part[MAP_NW][MAP_TK];
  const int r = blockIdx.x, k0 = blockIdx.y * MAP_TK, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  float* out = map + (long)r * map_bstride;
  const int key = k0 + tid;
  if (done && done[r] != 0) {  // (the same for every thread of the workgroup: nobody waits at a barrier below)
    if (key < Lk) out[key] = 0.f;
    return;
  }
  const T* qrow = q + (long)(r / q_div) * q_bstride;
  const T* krow = k + (long)(r / kv_group) * kv_bstride;
  float acc = 0.f;
  for (int h0 = 0; h0 < H; h0 += MAP_NW) {
    const int h = h0 + wave;
    if (h < H) {
      float qv[DK];
#pragma unroll
      for (int c = 0; c < DK; ++c) qv[c] = to_f32(qrow[(long)h * DK + c]);
      const T* kh = krow + (long)h * DK;
      const float* bh = bias_row ? bias_row + (long)h * bias_ld : nullptr;
      float st[MAP_KPL];
      float m = -INFINITY, l = 0.f;
      auto fold = [&](float s) {
        const float mn = fmaxf(m, s);
        l = l * __expf(m - mn) + __expf(s - mn);
        m = mn;
      };
#pragma unroll
      for (int i = 0; i < MAP_KPL; ++i) {  // the tile's keys: lane, lane + 64, ...
        const int j = k0 + i * 64 + lane;
        st[i] = -INFINITY;
        if (j < Lk) {
          float s = map_score<T, DK, VEC>(qv, kh + (long)j * ldk);
          if (bh) s += bh[j];
          st[i] = s;
          fold(s);
        }
      }
      for (int j = lane; j < Lk; j += 64) {  // every other key: the normaliser only
        if (j >= k0 && j < k0 + MAP_TK) continue;
        float s = map_score<T, DK, VEC>(qv, kh + (long)j * ldk);
        if (bh) s += bh[j];
        fold(s);
      }
      const float mw = wave_max(m);
      const float lw = wave_sum(m == -INFINITY ? 0.f : l * __expf(m - mw));
      const float il = 1.f / lw;
#pragma unroll
      for (int i = 0; i < MAP_KPL; ++i) part[wave][i * 64 + lane] = st[i] == -INFINITY ? 0.f : __expf(st[i] - mw) * il;
    }
    __syncthreads();
    const int nh = min(MAP_NW, H - h0);
    for (int w = 0; w < nh; ++w) acc += part[w][tid];  // heads h0 .. h0 + nh - 1, ascending
    __syncthreads();
  }
  if (key < Lk) out[key] = acc * (1.0f / (float)H);
}

template <typename T>
int launch_attn_map(const void* q, long q_bstride, int q_div, const void* k, long kv_bstride, long ldk, int kv_group, const float* bias_row,
                    long bias_ld, const int* done, float* map, long map_bstride, int R, int H, int Lk, int dk, hipStream_t s) {
  const bool vec = ((uintptr_t)k % 16 == 0) && (kv_bstride * (long)sizeof(T)) % 16 == 0 && (ldk * (long)sizeof(T)) % 16 == 0;
  const dim3 grid(R, (Lk + MAP_TK - 1) / MAP_TK);
#define MAP_LAUNCH(D)                                                                                                                  \
  if (vec)                                                                                                                             \
    hipLaunchKernelGGL((decode_attn_map_kernel<T, D, true>), grid, dim3(MAP_TK), 0, s, (const T*)q, q_bstride, q_div, (const T*)k,      \
                       kv_bstride, ldk, kv_group, bias_row, bias_ld, done, map, map_bstride, H, Lk);                                   \
  else                                                                                                                                 \
    hipLaunchKernelGGL((decode_attn_map_kernel<T, D, false>), grid, dim3(MAP_TK), 0, s, (const T*)q, q_bstride, q_div, (const T*)k,     \
                       kv_bstride, ldk, kv_group, bias_row, bias_ld, done, map, map_bstride, H, Lk)
  switch (dk) {
    case 8: MAP_LAUNCH(8); break;
    case 16: MAP_LAUNCH(16); break;
    case 32: MAP_LAUNCH(32); break;
    case 64: MAP_LAUNCH(64); break;
    case 128: MAP_LAUNCH(128); break;
    default: return KLAB_ERR_UNSUPPORTED;
  }
#undef MAP_LAUNCH
  KLAB_LAUNCH_CHECK();
  return KLAB_OK;
}
}  // namespace
}  // namespace klab

extern "C" int klab_t5_decode_attn_map(int dtype, const void* q, long q_bstride, int q_div, const void* k, long kv_bstride, long ldk,
                                       int kv_group, const float* bias_row, long bias_ld, const int* done, float* map, long map_bstride,
                                       int R, int H, int Lk, int dk, void* stream) {
  using namespace klab;
  if (!q || !k || !map || R <= 0 || H <= 0 || Lk <= 0 || q_div < 1 || kv_group < 1 || map_bstride < Lk || (bias_row && bias_ld < Lk))
    return KLAB_ERR_BADARG;
  if (((long)Lk + MAP_TK - 1) / MAP_TK > 65535) return KLAB_ERR_UNSUPPORTED;  // key tiles are the grid's y
  hipStream_t s = (hipStream_t)stream;
  if (dtype == KLAB_BF16)
    return launch_attn_map<bf16_t>(q, q_bstride, q_div, k, kv_bstride, ldk, kv_group, bias_row, bias_ld, done, map, map_bstride, R, H, Lk, dk, s);
  if (dtype == KLAB_F32)
    return launch_attn_map<float>(q, q_bstride, q_div, k, kv_bstride, ldk, kv_group, bias_row, bias_ld, done, map, map_bstride, R, H, Lk, dk, s);
  return KLAB_ERR_BADARG;
}
