// Fused multi-tensor Adafactor (math of transformers.optimization.Adafactor) for the trainable T5, with the compute-dtype
// shadow copy the Adam step also writes (adamw.hip, adam_step_kernel).  Four launches, whatever the number of tensors:
//
//   (a)  stats   g, p in            row sums / column partial sums of g^2 + eps0, sum p^2; R (and the 1-D tensors' V) updated
//   (a') reduce  partials in        column partials -> C (EMA folded in), mean(R), RMS(p), the factors rsqrt(R/mean R), rsqrt(C)
//   (b)  unorm   g in               sum u^2 per tile
//   (c)  apply   g, p (, m) in      u recomputed, clipped by RMS(u), scaled by lr_t; momentum, decay; p (, m) and the arena copy out
//
// 8 + 4 + 14 = 26 bytes per parameter without momentum (Adam: 30).  Everything that crosses workgroups goes through
// partials in a scratch buffer that are summed in a fixed order: there is no floating-point atomic in this file, and a step
// is a pure function of (gradients, parameters, state).  Nothing is read back by the host: t, beta2t and the relative step
// arrive by value, and whatever depends on RMS(p) / RMS(u) is computed on the device.
//
// Work unit = a TILE: whole rows of ONE tensor (about 16 K elements; more for very tall tensors so that a tensor has at most
// ~128 of them).  Row sums are therefore final inside the workgroup that owns the tile, and a tile's column sums are one
// partial row of the scratch buffer.  A workgroup finds its tensor by one binary search over the tensors' first-tile indices,
// which are copied to LDS first (the chain of dependent loads that held adam_step_kernel at 4.5 TB/s from global memory).
#include <math.h>

#include "common.h"
#include "klab_mm.h"
#include "multi_tensor.h"  // AfDesc

namespace klab {

struct AfHyper { float beta2t, omb2, eps0, eps1, rel, clip, beta1, omb1, wd; int scale_param, use_m; };

constexpr int AF_MAXD = 1024;     // tensors whose search keys fit the LDS copy (T5-large: ~560)
constexpr int AF_TILE = 16384;    // elements per tile (target)
constexpr int AF_TILES_PER_TENSOR = 128;
constexpr int AF_MAX_TILE_ROWS = 512;
constexpr int AF_ROWBUF = AF_MAX_TILE_ROWS * 4;  // per-row partials of up to 4 waves

// ---- 16-byte (W = 4, non-temporal) or scalar (W = 1) accesses --------------------------------------------------------------
template <int W> __device__ __forceinline__ void ldv(float* o, const float* p) {
  if constexpr (W == 4) {
    const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p));
    o[0] = v[0]; o[1] = v[1]; o[2] = v[2]; o[3] = v[3];
  } else {
    o[0] = *p;
  }
}
template <int W> __device__ __forceinline__ void ldc(float* o, const float* p) {  // cached (the factor vectors are re-read by every tile)
  if constexpr (W == 4) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(p);
    o[0] = v[0]; o[1] = v[1]; o[2] = v[2]; o[3] = v[3];
  } else {
    o[0] = *p;
  }
}
template <int W> __device__ __forceinline__ void stv(float* p, const float* v) {
  if constexpr (W == 4) __builtin_nontemporal_store(f32x4{v[0], v[1], v[2], v[3]}, reinterpret_cast<f32x4*>(p));
  else *p = v[0];
}
template <int W, typename T> __device__ __forceinline__ void st_arena(T* a, const float* v) {
  if constexpr (W == 4) {
    if constexpr (sizeof(T) == 2) *reinterpret_cast<bf16x4*>(a) = bf16x4{(bf16_t)v[0], (bf16_t)v[1], (bf16_t)v[2], (bf16_t)v[3]};
    else *reinterpret_cast<f32x4*>(a) = f32x4{v[0], v[1], v[2], v[3]};
  } else {
    *a = from_f32<T>(v[0]);
  }
}

// torch's `v.mul_(a).add_(x, alpha=b)`: the product v * a is rounded, then x * b is added with one rounding (ATen's vectorised
// add-with-alpha is a fused multiply-add).  Written with the _rn intrinsics so that the compiler contracts nothing else.
__device__ __forceinline__ float ema(float v, float a, float x, float b) { return __fmaf_rn(x, b, __fmul_rn(v, a)); }
__device__ __forceinline__ float sq_eps(float g, float eps0) { return __fadd_rn(__fmul_rn(g, g), eps0); }

// sum over the 256 threads, the same bits in every thread: xor-butterfly inside a wave, then the four waves in order
__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();  // red may still be read from an earlier call
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// which tensor owns `tile`: last descriptor with tile0 <= tile
__device__ __forceinline__ int af_find(const int* keys, const AfDesc* dglob, int nd, long tile) {
  int lo = 0, hi = nd - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    const long k = nd <= AF_MAXD ? (long)keys[mid] : dglob[mid].tile0;
    if (k <= tile) lo = mid; else hi = mid - 1;
  }
  return __builtin_amdgcn_readfirstlane(lo);
}

// the same search over the state offsets (af_reduce_kernel)
__device__ __forceinline__ int af_find_key(const int* keys, const AfDesc* dglob, int nd, long idx) {
  int lo = 0, hi = nd - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    const long k = nd <= AF_MAXD ? (long)keys[mid] : dglob[mid].soff;
    if (k <= idx) lo = mid; else hi = mid - 1;
  }
  return __builtin_amdgcn_readfirstlane(lo);
}

// how the 256 threads lie over a tile of `cols`-wide rows: LPR lanes per row (a power of two), 256 / LPR rows per sweep,
// J column steps of LPR * W when a row is wider than 256 * W.  A thread sees the same columns in every row of the tile.
struct Geo { int lpr, rpi, grp, l; };
template <int W> __device__ __forceinline__ Geo make_geo(int cols) {
  const int cpl = cols / W;
  int lpr = 1;
  while (lpr < cpl && lpr < 256) lpr <<= 1;
  Geo g; g.lpr = lpr; g.rpi = 256 / lpr; g.grp = threadIdx.x / lpr; g.l = threadIdx.x % lpr;
  return g;
}

enum { AF_STATS = 0, AF_UNORM = 1, AF_APPLY = 2 };

struct AfBufs {
  const float* grads; float* state; float* m; float* scal; float* fac; float* tsc; float* cpart; void* arena;
};

// per-tensor numbers of the apply pass, identical in every workgroup of the tensor
struct AfScal { float div, lr, wdlr; };

template <typename T, int W>
__device__ __forceinline__ void apply_unit(const AfHyper& h, const AfScal& sc, const float* u, float* pv, const float* mv, float* pptr, float* mptr,
                                           T* aptr) {
  float mo[W];
#pragma unroll
  for (int i = 0; i < W; ++i) {
    float x = u[i] / sc.div;  // update.div_(...): a true division, one rounding
    x = __fmul_rn(x, sc.lr);
    if (h.use_m) { mo[i] = ema(mv[i], h.beta1, x, h.omb1); x = mo[i]; }
    float p = pv[i];
    if (h.wd != 0.f) p = __fmaf_rn(p, sc.wdlr, p);
    pv[i] = p - x;
  }
  stv<W>(pptr, pv);
  if (h.use_m) stv<W>(mptr, mo);
  if (aptr) st_arena<W, T>(aptr, pv);
}

// One factored tile, rows [r0, r0 + nrow) of tensor d.
template <int PASS, typename T, int W, int J, int U>
__device__ void af_tile_factored(const AfDesc& d, long tile, int r0, int nrow, const AfBufs& b, const AfHyper& h, const AfScal& sc, float* rowbuf,
                                 float* colbuf, float* red) {
  const int cols = (int)d.cols;
  const Geo g = make_geo<W>(cols);
  const int wpr = g.lpr > 64 ? g.lpr / 64 : 1;
  const float* gbase = b.grads + d.goff + (long)r0 * cols;
  float* pbase = d.p + (long)r0 * cols;
  float* mbase = b.m ? b.m + d.goff + (long)r0 * cols : nullptr;
  T* abase = d.aoff < 0 ? nullptr : (T*)b.arena + d.aoff + (long)r0 * cols;
  const float* rfac = b.fac + d.soff + r0;
  float cacc[J][W];  // STATS: column sums of this thread's columns; otherwise rsqrt(C) of them
  float acc0 = 0.f;  // STATS: sum p^2; UNORM: sum u^2
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int c = (g.l + j * g.lpr) * W;
#pragma unroll
    for (int i = 0; i < W; ++i) cacc[j][i] = 0.f;
    if (PASS != AF_STATS && c < cols) ldc<W>(cacc[j], b.fac + d.soff + ((d.rows + 3) & ~3L) + c);
  }
  for (int base = 0; base < nrow; base += g.rpi * U) {
    float gv[U][J][W], pv[U][J][W], mv[U][J][W];
    bool ok[U][J];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int rl = base + u * g.rpi + g.grp;
#pragma unroll
      for (int j = 0; j < J; ++j) {
        const int c = (g.l + j * g.lpr) * W;
        ok[u][j] = rl < nrow && c < cols;
        if (ok[u][j]) {
          const long off = (long)rl * cols + c;
          ldv<W>(gv[u][j], gbase + off);
          if (PASS != AF_UNORM) ldv<W>(pv[u][j], pbase + off);
          if (PASS == AF_APPLY && h.use_m) ldv<W>(mv[u][j], mbase + off);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int rl = base + u * g.rpi + g.grp;
      if constexpr (PASS == AF_STATS) {
        float rs = 0.f;
#pragma unroll
        for (int j = 0; j < J; ++j)
          if (ok[u][j]) {
#pragma unroll
            for (int i = 0; i < W; ++i) {
              const float q = sq_eps(gv[u][j][i], h.eps0);
              rs += q; cacc[j][i] += q;
              acc0 += pv[u][j][i] * pv[u][j][i];
            }
          }
        for (int o = (g.lpr < 64 ? g.lpr : 64) >> 1; o > 0; o >>= 1) rs += __shfl_xor(rs, o, 64);
        if (rl < nrow && (g.l & 63) == 0) rowbuf[rl * wpr + (g.l >> 6)] = rs;
      } else {
        const float rf = rl < nrow ? rfac[rl] : 0.f;
#pragma unroll
        for (int j = 0; j < J; ++j)
          if (ok[u][j]) {
            float uu[W];
#pragma unroll
            for (int i = 0; i < W; ++i) uu[i] = (rf * cacc[j][i]) * gv[u][j][i];
            if constexpr (PASS == AF_UNORM) {
#pragma unroll
              for (int i = 0; i < W; ++i) acc0 += uu[i] * uu[i];
            } else {
              const long off = (long)rl * cols + (g.l + j * g.lpr) * W;
              apply_unit<T, W>(h, sc, uu, pv[u][j], mv[u][j], pbase + off, mbase ? mbase + off : nullptr, abase ? abase + off : nullptr);
            }
          }
      }
    }
  }
  if constexpr (PASS == AF_STATS) {
    // column partials of the tile: one owner per column when a row spans the workgroup, else the row groups are added in order
    float* cp = b.cpart + d.poff + (tile - d.tile0) * cols;
    if (g.rpi == 1) {
#pragma unroll
      for (int j = 0; j < J; ++j) {
        const int c = (g.l + j * g.lpr) * W;
        if (c < cols) {
#pragma unroll
          for (int i = 0; i < W; ++i) cp[c + i] = cacc[j][i];
        }
      }
    } else {
#pragma unroll
      for (int i = 0; i < W; ++i) colbuf[g.grp * (g.lpr * W) + g.l * W + i] = cacc[0][i];
    }
    __syncthreads();  // rowbuf and colbuf complete
    if (g.rpi > 1)
      for (int c = threadIdx.x; c < cols; c += 256) {
        float s = 0.f;
        for (int q = 0; q < g.rpi; ++q) s += colbuf[q * (g.lpr * W) + c];
        cp[c] = s;
      }
    // rows are whole inside the tile: the EMA into R happens here
    float rsum = 0.f;
    for (int rl = threadIdx.x; rl < nrow; rl += 256) {
      float s = rowbuf[rl * wpr];
      for (int w = 1; w < wpr; ++w) s += rowbuf[rl * wpr + w];
      float* R = b.state + d.soff + r0 + rl;
      const float rn = ema(*R, h.beta2t, s / (float)cols, h.omb2);
      *R = rn;
      rsum += rn;
    }
    const float p2 = block_sum(acc0, red);
    const float rs = block_sum(rsum, red);
    if (threadIdx.x == 0) { b.tsc[tile * 4 + 0] = p2; b.tsc[tile * 4 + 1] = rs; }
    __syncthreads();  // rowbuf / colbuf are reused by the workgroup's next tile
  } else if constexpr (PASS == AF_UNORM) {
    const float u2 = block_sum(acc0, red);
    if (threadIdx.x == 0) b.tsc[tile * 4 + 2] = u2;
  }
}

// One tile of an unfactored (1-D) tensor: elements [e0, e1), both multiples of 4 (the tensor's length is).
template <int PASS, typename T>
__device__ void af_tile_vector(const AfDesc& d, long tile, long e0, long e1, const AfBufs& b, const AfHyper& h, const AfScal& sc, float* red) {
  float acc = 0.f;
  for (long e = e0 + threadIdx.x * 4; e < e1; e += 1024) {
    float gv[4], vv[4], pv[4], mv[4], uu[4];
    ldv<4>(gv, b.grads + d.goff + e);
    ldc<4>(vv, b.state + d.soff + e);
    if (PASS != AF_UNORM) ldv<4>(pv, d.p + e);
    if constexpr (PASS == AF_STATS) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        vv[i] = ema(vv[i], h.beta2t, sq_eps(gv[i], h.eps0), h.omb2);
        acc += pv[i] * pv[i];
      }
      *reinterpret_cast<f32x4*>(b.state + d.soff + e) = f32x4{vv[0], vv[1], vv[2], vv[3]};
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) uu[i] = (1.f / sqrtf(vv[i])) * gv[i];
      if constexpr (PASS == AF_UNORM) {
#pragma unroll
        for (int i = 0; i < 4; ++i) acc += uu[i] * uu[i];
      } else {
        if (h.use_m) ldv<4>(mv, b.m + d.goff + e);
        apply_unit<T, 4>(h, sc, uu, pv, mv, d.p + e, b.m ? b.m + d.goff + e : nullptr, d.aoff < 0 ? nullptr : (T*)b.arena + d.aoff + e);
      }
    }
  }
  if constexpr (PASS != AF_APPLY) {
    const float s = block_sum(acc, red);
    if (threadIdx.x == 0) b.tsc[tile * 4 + (PASS == AF_STATS ? 0 : 2)] = s;
  }
}

template <int PASS, typename T>
__global__ __launch_bounds__(256) void af_tile_kernel(const AfDesc* __restrict__ dglob, int nd, long ntiles, AfBufs b, AfHyper h) {
  __shared__ int keys[AF_MAXD];
  __shared__ float rowbuf[PASS == AF_STATS ? AF_ROWBUF : 1];
  __shared__ float colbuf[PASS == AF_STATS ? 1024 : 1];
  __shared__ float red[4];
  if (nd <= AF_MAXD) {
    for (int i = threadIdx.x; i < nd; i += 256) keys[i] = (int)dglob[i].tile0;
    __syncthreads();
  }
  for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int ti = af_find(keys, dglob, nd, tile);
    const AfDesc d = dglob[ti];
    const long lt = tile - d.tile0;
    const long numel = d.factored ? d.rows * d.cols : d.cols;
    const long ntl = d.factored ? (d.rows + d.tile_len - 1) / d.tile_len : (numel + d.tile_len - 1) / d.tile_len;
    AfScal sc{1.f, 0.f, 0.f};
    if constexpr (PASS == AF_APPLY) {
      // RMS(u) of the tensor from its tiles' partials: every workgroup of the tensor adds them in the same order
      float s = 0.f;
      for (long t = threadIdx.x; t < ntl; t += 256) s += b.tsc[(d.tile0 + t) * 4 + 2];
      s = block_sum(s, red);
      const float rmsu = sqrtf(s) / sqrtf((float)numel);
      const float rmsp = b.scal[ti * 4 + 1];
      sc.div = fmaxf(1.f, rmsu / h.clip);
      sc.lr = h.rel * (h.scale_param ? fmaxf(h.eps1, rmsp) : 1.f);
      sc.wdlr = -h.wd * sc.lr;
      if (lt == 0 && threadIdx.x == 0) b.scal[ti * 4 + 2] = rmsu;
    }
    if (!d.factored) {
      const long e0 = lt * d.tile_len, e1 = e0 + d.tile_len < numel ? e0 + d.tile_len : numel;
      af_tile_vector<PASS, T>(d, tile, e0, e1, b, h, sc, red);
      continue;
    }
    const int r0 = (int)(lt * d.tile_len);
    const int nrow = (int)(d.rows - r0 < d.tile_len ? d.rows - r0 : d.tile_len);
    const int cols = (int)d.cols;
#define AF_CALL(W, J, U) af_tile_factored<PASS, T, W, J, U>(d, tile, r0, nrow, b, h, sc, rowbuf, colbuf, red)
    if ((cols & 3) == 0) {
      if (cols <= 1024) AF_CALL(4, 1, 4);
      else if (cols <= 2048) AF_CALL(4, 2, 2);
      else if (cols <= 4096) AF_CALL(4, 4, 1);
      else AF_CALL(4, 8, 1);
    } else {
      if (cols <= 256) AF_CALL(1, 1, 4);
      else AF_CALL(1, 8, 1);
    }
#undef AF_CALL
  }
}

// (a'): one thread per element of the flat R|C|V state.
__global__ __launch_bounds__(256) void af_reduce_kernel(const AfDesc* __restrict__ dglob, int nd, long state_elems, AfBufs b, AfHyper h) {
  __shared__ int keys[AF_MAXD];
  __shared__ float red[4];
  if (nd <= AF_MAXD) {
    for (int i = threadIdx.x; i < nd; i += 256) keys[i] = (int)dglob[i].soff;
    __syncthreads();
  }
  // A block owns 256 consecutive state elements, which belong to one tensor or to a few small ones.  Per tensor the block adds
  // the tiles' sum p^2 and sum R once, together (every block of the tensor in the same order: the same bits); the block that
  // holds the tensor's first element writes the per-tensor scalars.
  const long base = (long)blockIdx.x * 256, idx = base + threadIdx.x;
  const long last = base + 255 < state_elems ? base + 255 : state_elems - 1;
  const int first = af_find_key(keys, dglob, nd, base), last_t = af_find_key(keys, dglob, nd, last);
  int mine = -1;
  float mean_r = 1.f;
  for (int ti = first; ti <= last_t; ++ti) {
    const AfDesc d = dglob[ti];
    const long numel = d.factored ? d.rows * d.cols : d.cols;
    const long ntl = d.factored ? (d.rows + d.tile_len - 1) / d.tile_len : (numel + d.tile_len - 1) / d.tile_len;
    float s0 = 0.f, s1 = 0.f;
    for (long t = threadIdx.x; t < ntl; t += 256) {
      s0 += b.tsc[(d.tile0 + t) * 4 + 0];
      if (d.factored) s1 += b.tsc[(d.tile0 + t) * 4 + 1];
    }
    s0 = block_sum(s0, red);
    s1 = block_sum(s1, red);
    const float mr = d.factored ? s1 / (float)d.rows : 1.f;
    if (d.soff >= base && threadIdx.x == 0) {
      b.scal[ti * 4 + 0] = mr;
      b.scal[ti * 4 + 1] = sqrtf(s0) / sqrtf((float)numel);  // RMS(p) before the update
    }
    if (idx >= d.soff) { mine = ti; mean_r = mr; }
  }
  if (idx >= state_elems || mine < 0) return;
  const AfDesc d = dglob[mine];
  if (!d.factored) return;
  const long e = idx - d.soff;
  const long ntl = (d.rows + d.tile_len - 1) / d.tile_len;
  const long rows4 = (d.rows + 3) & ~3L;  // C starts on a 16-byte boundary
  if (e < d.rows) {
    b.fac[idx] = 1.f / sqrtf(b.state[idx] / mean_r);
  } else if (e >= rows4 && e - rows4 < d.cols) {
    const long c = e - rows4;
    const float* cp = b.cpart + d.poff + c;
    float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};  // eight loads in flight; tile t always lands in a[t % 8]
    long t = 0;
    for (; t + 8 <= ntl; t += 8) {
#pragma unroll
      for (int k = 0; k < 8; ++k) a[k] += cp[(t + k) * d.cols];
    }
    for (int k = 0; t < ntl; ++t, ++k) a[k] += cp[t * d.cols];
    const float s = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
    const float cn = ema(b.state[idx], h.beta2t, s / (float)d.rows, h.omb2);
    b.state[idx] = cn;
    b.fac[idx] = 1.f / sqrtf(cn);
  }
}

static long round_up4(long x) { return (x + 3) & ~3L; }

}  // namespace klab

using namespace klab;

extern "C" int klab_adafactor_plan(int n, const long* rows, const long* cols, const int* factored, long* out, long* totals) {
  if (n <= 0 || !rows || !cols || !factored || !out || !totals) return KLAB_ERR_BADARG;
  long soff = 0, tile = 0, poff = 0;
  for (int i = 0; i < n; ++i) {
    const long r = factored[i] ? rows[i] : 1, c = cols[i];
    if (r <= 0 || c <= 0) return KLAB_ERR_BADARG;
    const long numel = r * c;
    if (numel % 4 || numel >= (1L << 31)) return KLAB_ERR_UNSUPPORTED;
    long tl, ntl;
    if (factored[i]) {
      if (c > ((c & 3) ? 2048 : 8192)) return KLAB_ERR_UNSUPPORTED;
      tl = (AF_TILE + c - 1) / c;
      const long by_count = (r + AF_TILES_PER_TENSOR - 1) / AF_TILES_PER_TENSOR;
      if (by_count > tl) tl = by_count;
      tl = round_up4(tl);  // a tile starts on a 16-byte boundary whatever the row length
      if (tl > AF_MAX_TILE_ROWS) tl = AF_MAX_TILE_ROWS;
      ntl = (r + tl - 1) / tl;
    } else {
      tl = AF_TILE;
      ntl = (numel + tl - 1) / tl;
    }
    out[i * 4 + 0] = soff; out[i * 4 + 1] = tile; out[i * 4 + 2] = tl; out[i * 4 + 3] = factored[i] ? poff : 0;
    soff += factored[i] ? round_up4(r) + round_up4(c) : numel;  // R | C, each on a 16-byte boundary, or V
    tile += ntl;
    if (factored[i]) poff += ntl * c;
    if (soff >= (1L << 31) || tile >= (1L << 31)) return KLAB_ERR_UNSUPPORTED;
  }
  totals[0] = soff; totals[1] = tile; totals[2] = soff + 4 * tile + poff; totals[3] = 4L * n;
  return KLAB_OK;
}

extern "C" int klab_adafactor_step(const void* desc_dev, int ndesc, long state_elems, long ntiles, const float* grads, float* state, float* m,
                                   float* scalars, float* scratch, void* arena, int dtype, float beta2t, float one_minus_beta2t, float eps0,
                                   float eps1, float rel_step, float clip_threshold, float beta1, float one_minus_beta1, float weight_decay,
                                   int scale_parameter, void* stream) {
  if (!desc_dev || ndesc <= 0 || state_elems <= 0 || ntiles <= 0 || !grads || !state || !scalars || !scratch || !arena ||
      !(clip_threshold > 0.f) || (dtype != KLAB_BF16 && dtype != KLAB_F32))
    return KLAB_ERR_BADARG;
  const bool use_m = m != nullptr;
  if (use_m && !(beta1 >= 0.f)) return KLAB_ERR_BADARG;
  AfHyper h{beta2t, one_minus_beta2t, eps0, eps1, rel_step, clip_threshold, use_m ? beta1 : 0.f, use_m ? one_minus_beta1 : 1.f, weight_decay,
            scale_parameter, use_m ? 1 : 0};
  AfBufs b{grads, state, m, scalars, scratch, scratch + state_elems, scratch + state_elems + 4 * ntiles, arena};
  const AfDesc* d = (const AfDesc*)desc_dev;
  hipStream_t s = (hipStream_t)stream;
  constexpr long AF_GRID = 2048;  // 256 CUs x 8 workgroups
  const unsigned gt = (unsigned)(ntiles < AF_GRID ? ntiles : AF_GRID);
  const unsigned gr = (unsigned)((state_elems + 255) / 256);  // one block per 256 state elements (state_elems < 2^31)
  hipLaunchKernelGGL((af_tile_kernel<AF_STATS, float>), dim3(gt), dim3(256), 0, s, d, ndesc, ntiles, b, h);
  hipLaunchKernelGGL(af_reduce_kernel, dim3(gr), dim3(256), 0, s, d, ndesc, state_elems, b, h);
  hipLaunchKernelGGL((af_tile_kernel<AF_UNORM, float>), dim3(gt), dim3(256), 0, s, d, ndesc, ntiles, b, h);
  if (dtype == KLAB_BF16) hipLaunchKernelGGL((af_tile_kernel<AF_APPLY, bf16_t>), dim3(gt), dim3(256), 0, s, d, ndesc, ntiles, b, h);
  else hipLaunchKernelGGL((af_tile_kernel<AF_APPLY, float>), dim3(gt), dim3(256), 0, s, d, ndesc, ntiles, b, h);
  KLAB_LAUNCH_CHECK();
  return KLAB_OK;
}
