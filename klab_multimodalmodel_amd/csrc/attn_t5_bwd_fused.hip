// Back half of a T5 attention sub-layer (backward) in ONE launch, one workgroup per (sample, head): the o / co projection dgrad
// (HF/t5:209 + 369 / 432, backward), delta = rowsum(dO * O), and the attention core's backward (HF/t5:144-173) in a single pass
// over the scores.  For d_model = 512, head dim 64, H * dk = 512 and at most 64 queries / keys per sample (T5-small at the caption
// shapes: Le = 58, Lt = 64).  Replaces two launches of the serial chain (the projection klab_gemm into dctx, t5_attn_bwd_mfma):
//   a. dO_h = dy[sample rows, :] . W[:, h*64 : h*64+64], K = 512, computed "swapped" (A = W^T slice, B = dy^T), so a lane ends up
//      with one query and four consecutive head columns.  Both operands stream through LDS in k-tiles of 64 (slot = W rows [64][64]
//      and dy rows [64][64], 16-B chunk c of row r at c ^ (r & 7): conflict-free transposed reads of W), three k-tiles in flight in
//      registers, two slots; dO is rounded to bf16 (as the GEMM's output was) and only ever
//      lives in the dO image.  delta from the rounded values and the forward's context rows;
//   b. one pass: wave w owns queries 16 w .. + 15 against all keys -- S^T and dP^T tiles (A = K / V rows, B = Q / dO rows), P from
//      the forward's log-sum-exp, the dropout mask (the forward's (seed, tag, slab b*H + h, q*Lk + key) hash), dS; dQ^T = K^T dS^T
//      accumulated in registers; P*mask and dS go to LDS images [query][key] (and dS to the caller's scratch, t5_attn_bwd_mfma's
//      layout); one barrier;
//   c. wave w owns keys 16 w .. + 15: dV^T = dO^T (P*mask) and dK^T = Q^T dS, every operand a transposed read of an image.
// What t5_attn_bwd_mfma computed twice (S, the bias look-up, exp, the hash, dP, dS: once per orientation) is computed once here.
// LDS: Q, K, V, dO images (TrImg layout, 11 KiB each) + the two k-tile slots (32 KiB), which the P*mask / dS images alias after
// phase a: 76 KiB, two workgroups per CU.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "common.h"
#include "klab_mm.h"

namespace klab {

int dbias_reduce_dispatch(const void* ds_ws, float* dbias, int nbatch, int H, int Lq, int Lk, hipStream_t s);

namespace abf {

constexpr int D = 512, DK = 64, KT = 64, NKT = D / KT, SLOT = 16384, NSLOT = 2, NBUF = 3;
// 64-column image, rows = the index a transposed read contracts over: 8-row groups of 160-B rows displaced by 128 B
// (ds_read_b64_tr_b16 conflict-free; the same layout as attn_t5_mfma.hip's TrImg<64>).  Plain 16-B row reads work on it as well.
constexpr int PITCHB = 160, GROUPB = 8 * PITCHB + 128, IMG = 8 * GROUPB;
__device__ __forceinline__ int off(int row, int col) { return (row >> 3) * GROUPB + (row & 7) * PITCHB + col * 2; }

typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4_t;
__device__ __forceinline__ bf16x4 tr4(const char* p) { return __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_t*)p); }

// MFMA operand for a product that sums over the image's ROW index: rows row0 .. + 31, output index col0 + (lane & 15), k order
// kappa(g, j) = 16 (j >> 2) + 4 g + (j & 3) -- the order of an accumulator tile pair packed with pack8
__device__ __forceinline__ bf16x8 tr_frag(const char* img, int row0, int col0, int lane) {
  const int g = lane >> 4, q4 = (lane & 15) >> 2, pp = lane & 3;
  const int r = row0 + 4 * g + q4;
  const bf16x4 lo = tr4(img + off(r, col0 + 4 * pp)), hi = tr4(img + off(r + 16, col0 + 4 * pp));
  return bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}
// plain row fragment: row r, columns 32 ks + 8 (lane >> 4) .. + 7
__device__ __forceinline__ bf16x8 row_frag(const char* img, int r, int ks, int lane) {
  return *reinterpret_cast<const bf16x8*>(img + off(r, ks * 32 + (lane >> 4) * 8));
}
__device__ __forceinline__ bf16x8 pack8(const f32x4& a, const f32x4& b) {
  return bf16x8{(bf16_t)a[0], (bf16_t)a[1], (bf16_t)a[2], (bf16_t)a[3], (bf16_t)b[0], (bf16_t)b[1], (bf16_t)b[2], (bf16_t)b[3]};
}

struct P {
  const bf16_t* dy; long lddy;
  const bf16_t* w;  // [512, 512]: row n, head h's columns h*64 .. + 63
  const bf16_t* q; long ldq; const bf16_t* k; long ldk; const bf16_t* v; long ldv;
  const bf16_t* ctx; long ldo; const float* lse;
  const float* bias; int causal;
  int B, H, Lq, Lk;
  float p; const uint32_t* seed; uint32_t tag;
  bf16_t* dq; long lddq; bf16_t* dkk; long lddk; bf16_t* dv; long lddv;
  float* dbias; bf16_t* ds_ws;
};

__global__ __launch_bounds__(256, 2) void t5_attn_bwd_fused(P p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* Qi = smem;
  char* Ki = Qi + IMG;
  char* Vi = Ki + IMG;
  char* dOi = Vi + IMG;
  char* ring = dOi + IMG;  // NSLOT x SLOT; after phase a: the P*mask and dS images
  char* PDi = ring;
  char* dSi = ring + IMG;
  const int Lq = p.Lq, Lk = p.Lk, H = p.H;
  // workgroup -> (sample, head): the heads of a sample get block ids equal mod 8 (one XCD, one L2 for its dy rows) -- as
  // t5_attn_fused_fwd; speed only
  int b, h;
  {
    const int i = blockIdx.x;
    if ((p.B & 7) == 0) { const int xcd = i & 7, kk = i >> 3; h = kk % H; b = (kk / H) * 8 + xcd; }
    else { b = i / H; h = i % H; }
  }
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4;
  const int q0 = wave * 16, q = q0 + (lane & 15), qc = q < Lq ? q : Lq - 1;

  // ring k-tile kt: W rows kt*64 .. + 63 (head h's 128-byte column slice) and the sample's dy rows, columns kt*64 .. + 63; thread
  // tid + 256 u loads row (tid + 256 u) >> 3, 16-byte chunk tid & 7 of both (eight lanes per 128-byte row segment)
  const bf16_t* wsrc[2];
  const bf16_t* dysrc[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int r = (tid + u * 256) >> 3, c = tid & 7;
    wsrc[u] = p.w + (long)r * D + h * DK + c * 8;
    dysrc[u] = p.dy + ((long)b * Lq + (r < Lq ? r : Lq - 1)) * p.lddy + c * 8;  // rows past the sequence: a copy, zeroed below
  }
  bf16x8 rw[NBUF][2], rd[NBUF][2];
  auto load_tile = [&](int kt, int sb) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      rw[sb][u] = *reinterpret_cast<const bf16x8*>(wsrc[u] + (long)kt * KT * D);
      rd[sb][u] = *reinterpret_cast<const bf16x8*>(dysrc[u] + kt * KT);
    }
  };
  auto store_tile = [&](int sb, char* st) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int r = (tid + u * 256) >> 3, pos = ((tid & 7) ^ (r & 7)) * 16;
      *reinterpret_cast<bf16x8*>(st + r * 128 + pos) = rw[sb][u];
      *reinterpret_cast<bf16x8*>(st + 8192 + r * 128 + pos) = rd[sb][u];
    }
  };

  // everything else phase b reads from memory, requested first: Q / K / V images (rows past the sequence zero), the lane's 16
  // position-bias values, its query's log-sum-exp, its context columns for delta
  bf16x8 vq[2], vk[2], vv[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int ch = tid + u * 256, r = ch >> 3, c = (ch & 7) * 8;
    vq[u] = bf16x8{}; vk[u] = bf16x8{}; vv[u] = bf16x8{};
    if (r < Lq) vq[u] = *reinterpret_cast<const bf16x8*>(p.q + ((long)b * Lq + r) * p.ldq + h * DK + c);
    if (r < Lk) {
      vk[u] = *reinterpret_cast<const bf16x8*>(p.k + ((long)b * Lk + r) * p.ldk + h * DK + c);
      vv[u] = *reinterpret_cast<const bf16x8*>(p.v + ((long)b * Lk + r) * p.ldv + h * DK + c);
    }
  }
  f32x4 bv[4];
  {
    const float* brow = p.bias ? p.bias + ((long)h * Lq + qc) * Lk : nullptr;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = t * 16 + g * 4 + r;
        bv[t][r] = brow ? brow[key < Lk ? key : Lk - 1] : 0.f;
      }
  }
  const float lq = q < Lq ? p.lse[((long)b * H + h) * Lq + q] : INFINITY;  // padded queries: P = exp(-inf) = 0
  bf16x4 ov[4];
#pragma unroll
  for (int jt = 0; jt < 4; ++jt) ov[jt] = *reinterpret_cast<const bf16x4*>(p.ctx + ((long)b * Lq + qc) * p.ldo + h * DK + jt * 16 + g * 4);
#pragma unroll
  for (int i = 0; i < NBUF; ++i) load_tile(i, i);
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int ch = tid + u * 256, r = ch >> 3, c = (ch & 7) * 8;
    *reinterpret_cast<bf16x8*>(Qi + off(r, c)) = vq[u];
    *reinterpret_cast<bf16x8*>(Ki + off(r, c)) = vk[u];
    *reinterpret_cast<bf16x8*>(Vi + off(r, c)) = vv[u];
  }

  // ---- a. dO^T[j][q] = sum_n W[n][h*64 + j] dy[q][n]: acc[jt][r] = dO[q][16 jt + 4 g + r] ----
  // NBUF k-tiles in flight in registers (an LDS-DMA ring makes hipcc wait for every outstanding DMA before each LDS read), two
  // LDS slots, one barrier per k-tile
  f32x4 acc[4];
#pragma unroll
  for (int jt = 0; jt < 4; ++jt) acc[jt] = f32x4{0.f, 0.f, 0.f, 0.f};
  {
    const int q4 = (lane & 15) >> 2, pp = lane & 3;
    const int ql = wave * 16 + (lane & 15);  // dy row of the lane's query
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
      char* st = ring + (kt & 1) * SLOT;
      store_tile(kt % NBUF, st);
      if (kt + NBUF < NKT) load_tile(kt + NBUF, kt % NBUF);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      const char* Ws = st;
      const char* Ds = st + 8192;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const int c0 = 4 * ks + (g >> 1);
        const bf16x4 dlo = *reinterpret_cast<const bf16x4*>(Ds + ql * 128 + ((c0 ^ (ql & 7)) * 16) + (g & 1) * 8);
        const bf16x4 dhi = *reinterpret_cast<const bf16x4*>(Ds + ql * 128 + (((c0 + 2) ^ (ql & 7)) * 16) + (g & 1) * 8);
        const bf16x8 dyf = bf16x8{dlo[0], dlo[1], dlo[2], dlo[3], dhi[0], dhi[1], dhi[2], dhi[3]};
        const int r = ks * 32 + 4 * g + q4;
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) {
          const int chunk = 2 * jt + (pp >> 1);
          const bf16x4 lo = tr4(Ws + r * 128 + ((chunk ^ (r & 7)) * 16) + (pp & 1) * 8);
          const bf16x4 hi = tr4(Ws + (r + 16) * 128 + ((chunk ^ (r & 7)) * 16) + (pp & 1) * 8);
          const bf16x8 wf = bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
          acc[jt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, dyf, acc[jt], 0, 0, 0);
        }
      }
    }
  }
  // dO rounded to bf16 (the GEMM's output rounding) -> dO image; delta[q] = sum_j dO[q][j] O[q][j] from the rounded values
  float delta;
  {
    float a = 0.f;
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) {
      bf16x4 o = bf16x4{(bf16_t)acc[jt][0], (bf16_t)acc[jt][1], (bf16_t)acc[jt][2], (bf16_t)acc[jt][3]};
      if (q >= Lq) o = bf16x4{};
#pragma unroll
      for (int r = 0; r < 4; ++r) a += (float)o[r] * (float)ov[jt][r];
      *reinterpret_cast<bf16x4*>(dOi + off(q, jt * 16 + g * 4)) = o;
    }
    a += __shfl_xor(a, 16, 64);
    a += __shfl_xor(a, 32, 64);
    delta = a;
  }
  __syncthreads();  // ring done (it becomes the P*mask / dS images); Q / K / V / dO images complete

  // ---- b. one pass over the scores: the wave's 16 queries against all keys -> dQ, P*mask and dS images ----
  const DropCtx dc = drop_slab(make_drop(p.seed, p.tag, p.p), (uint32_t)(b * H + h));
  const int Lkp = (Lk + 31) & ~31, NS = Lkp / 32;
  {
    bf16x8 qf[2], dof[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) { qf[ks] = row_frag(Qi, q, ks, lane); dof[ks] = row_frag(dOi, q, ks, lane); }
    float* dbrow = (p.dbias && !p.ds_ws && q < Lq) ? p.dbias + ((long)h * Lq + q) * Lk : nullptr;
    bf16_t* dsrow = (p.ds_ws && q < Lq) ? p.ds_ws + (((long)b * H + h) * Lq + q) * Lkp : nullptr;
    f32x4 dqa[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) dqa[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int sidx = 0; sidx < 2; ++sidx) {
      if (sidx < NS) {
        f32x4 pd2[2], ds2[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const int t = 2 * sidx + u;
          f32x4 st = {0.f, 0.f, 0.f, 0.f}, dpt = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) {
            st = __builtin_amdgcn_mfma_f32_16x16x32_bf16(row_frag(Ki, t * 16 + (lane & 15), ks, lane), qf[ks], st, 0, 0, 0);
            dpt = __builtin_amdgcn_mfma_f32_16x16x32_bf16(row_frag(Vi, t * 16 + (lane & 15), ks, lane), dof[ks], dpt, 0, 0, 0);
          }
          // st[r] = S[q][key = 16 t + 4 g + r]
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int key = t * 16 + g * 4 + r;
            const bool ok = key < Lk && q < Lq && !(p.causal && key > q);
            const float pr = ok ? __expf(st[r] + bv[t][r] - lq) : 0.f;
            const float mlt = drop_mult32_nb(dc, (uint32_t)q * (uint32_t)Lk + key);
            const float dsv = pr * (dpt[r] * mlt - delta);
            if (dbrow) { if (ok) atomicAdd(dbrow + key, dsv); }
            pd2[u][r] = pr * mlt;
            ds2[u][r] = dsv;
          }
        }
        const bf16x8 pdf = pack8(pd2[0], pd2[1]), dsf = pack8(ds2[0], ds2[1]);
        const bf16x4 ds_lo = bf16x4{dsf[0], dsf[1], dsf[2], dsf[3]}, ds_hi = bf16x4{dsf[4], dsf[5], dsf[6], dsf[7]};
        *reinterpret_cast<bf16x4*>(PDi + off(q, sidx * 32 + g * 4)) = bf16x4{pdf[0], pdf[1], pdf[2], pdf[3]};
        *reinterpret_cast<bf16x4*>(PDi + off(q, sidx * 32 + 16 + g * 4)) = bf16x4{pdf[4], pdf[5], pdf[6], pdf[7]};
        *reinterpret_cast<bf16x4*>(dSi + off(q, sidx * 32 + g * 4)) = ds_lo;
        *reinterpret_cast<bf16x4*>(dSi + off(q, sidx * 32 + 16 + g * 4)) = ds_hi;
        if (dsrow) {  // dS tile pair for the batch reduction (keys 32 s + 4 g .. and + 16): t5_attn_bwd_mfma's layout
          *reinterpret_cast<bf16x4*>(dsrow + sidx * 32 + g * 4) = ds_lo;
          *reinterpret_cast<bf16x4*>(dsrow + sidx * 32 + 16 + g * 4) = ds_hi;
        }
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) dqa[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_frag(Ki, sidx * 32, dt * 16, lane), dsf, dqa[dt], 0, 0, 0);
      }
    }
    if (q < Lq) {
#pragma unroll
      for (int dt = 0; dt < 4; ++dt)
        *reinterpret_cast<bf16x4*>(p.dq + ((long)b * Lq + q) * p.lddq + h * DK + dt * 16 + g * 4) =
            bf16x4{(bf16_t)dqa[dt][0], (bf16_t)dqa[dt][1], (bf16_t)dqa[dt][2], (bf16_t)dqa[dt][3]};
    }
  }
  __syncthreads();

  // ---- c. the wave's 16 keys: dV^T = dO^T (P*mask), dK^T = Q^T dS (sums over the queries) ----
  const int k0 = wave * 16;
  if (k0 >= Lk) return;
  const int NQS = (Lq + 31) / 32;  // query rows past the sequence are zero in both images
  f32x4 av[4], ak[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) { av[dt] = f32x4{0.f, 0.f, 0.f, 0.f}; ak[dt] = f32x4{0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
  for (int sidx = 0; sidx < 2; ++sidx) {
    if (sidx < NQS) {
      const bf16x8 pf = tr_frag(PDi, sidx * 32, k0, lane), sf = tr_frag(dSi, sidx * 32, k0, lane);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        av[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_frag(dOi, sidx * 32, dt * 16, lane), pf, av[dt], 0, 0, 0);
        ak[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_frag(Qi, sidx * 32, dt * 16, lane), sf, ak[dt], 0, 0, 0);
      }
    }
  }
  const int key = k0 + (lane & 15);
  if (key < Lk) {
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      const int dd = h * DK + dt * 16 + g * 4;
      *reinterpret_cast<bf16x4*>(p.dv + ((long)b * Lk + key) * p.lddv + dd) = bf16x4{(bf16_t)av[dt][0], (bf16_t)av[dt][1], (bf16_t)av[dt][2], (bf16_t)av[dt][3]};
      *reinterpret_cast<bf16x4*>(p.dkk + ((long)b * Lk + key) * p.lddk + dd) = bf16x4{(bf16_t)ak[dt][0], (bf16_t)ak[dt][1], (bf16_t)ak[dt][2], (bf16_t)ak[dt][3]};
    }
  }
}

}  // namespace abf
}  // namespace klab

using namespace klab;

extern "C" int klab_t5_attn_bwd_fused(const klab_attn_bwd_fused_args* fb, void* stream) {
  if (!fb) return KLAB_ERR_BADARG;
  const klab_attn_args* a = &fb->attn;
  if (!fb->dy || !fb->w || !a->q || !a->k || !a->v || !a->ctx || !a->lse || !a->dq || !a->dk_out || !a->dv) return KLAB_ERR_BADARG;
  if (a->B <= 0) return KLAB_OK;
  if (a->dtype != KLAB_BF16 || fb->d_model != abf::D || a->dk != abf::DK || a->H * a->dk != abf::D) return KLAB_ERR_UNSUPPORTED;
  if (a->Lq < 1 || a->Lq > 64 || a->Lk < 1 || a->Lk > 64 || a->score_scale || a->bias_mod) return KLAB_ERR_UNSUPPORTED;
  // 16-B row loads (dy / W through the ring, q / k / v), 8-B context loads and output stores
  auto al = [](const void* p, long ld, int elems) { return ((uintptr_t)p % (elems * 2)) == 0 && ld % elems == 0; };
  if (!al(fb->dy, fb->lddy, 8) || fb->lddy < abf::D || !al(fb->w, 0, 8) || !al(a->q, a->ldq, 8) || !al(a->k, a->ldk, 8) ||
      !al(a->v, a->ldv, 8) || !al(a->ctx, a->ldo, 4) || !al(a->dq, a->lddq, 4) || !al(a->dk_out, a->lddk, 4) || !al(a->dv, a->lddv, 4))
    return KLAB_ERR_UNSUPPORTED;
  if (a->ds_ws && ((uintptr_t)a->ds_ws & 7)) return KLAB_ERR_UNSUPPORTED;
  abf::P p;
  p.dy = (const bf16_t*)fb->dy; p.lddy = fb->lddy; p.w = (const bf16_t*)fb->w;
  p.q = (const bf16_t*)a->q; p.ldq = a->ldq; p.k = (const bf16_t*)a->k; p.ldk = a->ldk; p.v = (const bf16_t*)a->v; p.ldv = a->ldv;
  p.ctx = (const bf16_t*)a->ctx; p.ldo = a->ldo; p.lse = a->lse; p.bias = a->bias; p.causal = a->causal;
  p.B = a->B; p.H = a->H; p.Lq = a->Lq; p.Lk = a->Lk; p.p = a->drop_p; p.seed = a->seed_dev; p.tag = a->drop_tag;
  p.dq = (bf16_t*)a->dq; p.lddq = a->lddq; p.dkk = (bf16_t*)a->dk_out; p.lddk = a->lddk; p.dv = (bf16_t*)a->dv; p.lddv = a->lddv;
  p.dbias = a->dbias; p.ds_ws = (bf16_t*)a->ds_ws;
  hipStream_t s = (hipStream_t)stream;
  const size_t lds = 4 * (size_t)abf::IMG + abf::NSLOT * (size_t)abf::SLOT;
  int rc = ensure_dyn_lds(reinterpret_cast<const void*>(abf::t5_attn_bwd_fused), lds);
  if (rc) return rc;
  hipLaunchKernelGGL(abf::t5_attn_bwd_fused, dim3(a->B * a->H), dim3(256), lds, s, p);
  KLAB_LAUNCH_CHECK();
  if (a->dbias && a->ds_ws && !a->ds_defer) return dbias_reduce_dispatch(a->ds_ws, a->dbias, a->B, a->H, a->Lq, a->Lk, s);
  return KLAB_OK;
}
