// klab_gemm: C[M,N] = epilogue(alpha * sum_k A(m,k) * B(n,k)) on gfx950 matrix cores.
//
// One LDS-tiled MFMA kernel serves every dense contraction of the path (SURVEY §2.4 K1,K5,K11-K14
// and their dgrad/wgrad): operands are addressed as logical A[M,K], B[N,K]; each may be stored
// K-major ("NT" torch Linear forward: x[M,K], W[N,K]) or row-major-over-the-other-dim ("m-major":
// element (r,k) at base[k*ld + r]), which gives the NN (dgrad) and TN (wgrad) forms without
// transposed copies -- the stager transposes 16-byte chunks in registers on the way into LDS.
//   bf16: v_mfma_f32_16x16x32_bf16, fp32 accumulate.   fp32: v_mfma_f32_16x16x4_f32 (exact f32 FMA
//   chain; used by the parity mode).  The B tile is fed as the MFMA "A" operand so that each lane's
//   four accumulator registers are four CONSECUTIVE n of one m: the epilogue stores 8/16 B per lane.
// Epilogue (all optional, in this order): *alpha(*alpha_dev) -> +bias[n] -> act (relu | erf-gelu)
//   -> *gelu'(aux) or *(aux!=0)*aux_scale (backward of gelu / of relu+dropout) -> dropout(seed,tag,p)
//   -> +residual -> (+C if accumulate) -> store as f32 or as the input dtype.
#include <stdlib.h>

#include <map>
#include <mutex>
#include <vector>

#include "common.h"
#include <type_traits>
#include <utility>
#include "klab_mm.h"
#include "gemm_shared.h"
#include "multi_tensor.h"

#ifndef KLAB_GLDS_STAGES
#define KLAB_GLDS_STAGES 4
#endif

namespace klab {

template <typename T> struct MmaTraits;
template <> struct MmaTraits<bf16_t> {
  static constexpr int BK = 64;   // elements per K tile (128 B)
  static constexpr int KSTEP = 32;
};
template <> struct MmaTraits<float> {
  static constexpr int BK = 32;   // 128 B
  static constexpr int KSTEP = 4;
};


constexpr int ROWB = 144;  // K-major LDS row pitch in bytes: 128 B of K + one 16-B pad (conflict-free b128 reads)

// ---- LDS image of an m-major bf16 operand tile (contraction dim is the SLOW global dim) ------------
// The tile is kept exactly as it is loaded -- rows = 64 k's, columns = ROWS m's (16-B chunks of 8 m go
// in with one ds_write_b128) -- and the MFMA fragments come out through ds_read_b64_tr_b16, the gfx950
// hardware transpose read: per 16-lane group a 4(k) x 16(m) block is delivered so that lane i holds
// 4 consecutive k of column m0+i, i.e. half of the 16x16x32 A/B fragment.  Bank-conflict-free placement:
// row pitch PD dwords with PD/8 odd (k&7 -> eight distinct 8-dword slots) and every group of 8 k-rows
// displaced by 32 more dwords, so the two groups a 32-lane half touches (k-rows 8g.. and 8g+8..) split
// the 64 banks between them.
template <int ROWS> struct TrLayout {
  static constexpr int PD = (ROWS == 128) ? 72 : (ROWS == 64 ? 40 : 24);  // dwords; >= ROWS/2, PD/8 odd
  static constexpr int PITCHB = PD * 4;
  static constexpr int GROUPB = (8 * PD + 32) * 4;  // bytes per group of 8 k-rows
  static constexpr int BYTES = 8 * GROUPB;          // 64 k-rows
};

template <typename T, int ROWS, bool KMAJOR> struct TileBytes { static constexpr int value = ROWS * ROWB; };
template <int ROWS> struct TileBytes<bf16_t, ROWS, false> { static constexpr int value = TrLayout<ROWS>::BYTES; };

// stage one operand tile (ROWS x BK) from global into registers, then into LDS
template <typename T, int ROWS, bool KMAJOR>
struct Stager {
  using V = typename Vec16<T>::type;
  static constexpr int VEC = Vec16<T>::N;
  static constexpr int BK = MmaTraits<T>::BK;
  static constexpr int NCH = ROWS * 8 / 256;             // 16-B chunks per thread
  static constexpr int KPT = ROWS * BK / (256 * VEC);    // fp32 m-major: k's per thread (== NCH)
  static constexpr bool TR = (!KMAJOR) && sizeof(T) == 2;
  V v[NCH];

  __device__ __forceinline__ void load(const T* __restrict__ base, long ld, int row0, int k0, int nrows, int kend, int tid) {
    if constexpr (KMAJOR) {
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        int ch = tid + c * 256;
        int r = ch >> 3, kc = ch & 7;
        int gr = row0 + r, gk = k0 + kc * VEC;
        // unconditional load from a clamped in-range address + select: no branch per load
        const bool ok = gr < nrows && gk < kend;
        const int grc = gr < nrows ? gr : nrows - 1, gkc = gk < kend ? gk : kend - VEC;
        V z = *reinterpret_cast<const V*>(base + (long)grc * ld + gkc);
        if (!ok) z = V{};
        v[c] = z;
      }
    } else if constexpr (TR) {
      constexpr int CPR = ROWS / 8;  // chunks per k-row
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        int ch = tid + c * 256;
        int kk = ch / CPR, m8 = ch % CPR;
        int gk = k0 + kk, gr = row0 + m8 * 8;
        const bool ok = gr < nrows && gk < kend;
        const int grc = gr < nrows ? gr : nrows - 8, gkc = gk < kend ? gk : kend - 1;
        V z = *reinterpret_cast<const V*>(base + (long)gkc * ld + grc);
        if (!ok) z = V{};
        v[c] = z;
      }
    } else {
      constexpr int RG = ROWS / VEC;  // row groups
      int rg = tid % RG, kg = tid / RG;
      int gr = row0 + rg * VEC;
#pragma unroll
      for (int c = 0; c < KPT; ++c) {
        int gk = k0 + kg * KPT + c;
        const bool ok = gr < nrows && gk < kend;
        const int grc = gr < nrows ? gr : nrows - VEC, gkc = gk < kend ? gk : kend - 1;
        V z = *reinterpret_cast<const V*>(base + (long)gkc * ld + grc);
        if (!ok) z = V{};
        v[c] = z;
      }
    }
  }
  __device__ __forceinline__ void store(char* lds, int tid) const {
    if constexpr (KMAJOR) {
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        int ch = tid + c * 256;
        int r = ch >> 3, kc = ch & 7;
        *reinterpret_cast<V*>(lds + r * ROWB + kc * 16) = v[c];
      }
    } else if constexpr (TR) {
      constexpr int CPR = ROWS / 8;
      using TL = TrLayout<ROWS>;
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        int ch = tid + c * 256;
        int kk = ch / CPR, m8 = ch % CPR;
        *reinterpret_cast<V*>(lds + (kk >> 3) * TL::GROUPB + (kk & 7) * TL::PITCHB + m8 * 16) = v[c];
      }
    } else {
      constexpr int RG = ROWS / VEC;
      int rg = tid % RG, kg = tid / RG;
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        T* dst = reinterpret_cast<T*>(lds + (rg * VEC + i) * ROWB) + kg * KPT;
#pragma unroll
        for (int c = 0; c < KPT; ++c) dst[c] = v[c][i];
      }
    }
  }
};

// bf16 fragment (8 consecutive k of one row) for k-step ks of 32, row r0 + (lane & 15)
template <int ROWS, bool KMAJOR>
__device__ __forceinline__ bf16x8 load_frag_bf16(const char* tile, int r0, int ks, int lane) {
  if constexpr (KMAJOR) {
    return *reinterpret_cast<const bf16x8*>(tile + (r0 + (lane & 15)) * ROWB + ks * 64 + (lane >> 4) * 16);
  } else {
    using TL = TrLayout<ROWS>;
    typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;
    const int q = (lane & 15) >> 2, pp = lane & 3;
    const char* base = tile + (ks * 4 + (lane >> 4)) * TL::GROUPB + q * TL::PITCHB + (r0 + 4 * pp) * 2;
    bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(base));
    bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(base + 4 * TL::PITCHB));
    return bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  }
}



// ---- bf16 fast path: asynchronous global->LDS ring (all four operand layouts) -------------------------
// The register-staged loop further down exposes one full memory latency (~1 us under load) per k-tile; here
// S = 4 stages of BK = 32 live in LDS and are filled by global_load_lds_dwordx4 (LDS-DMA: no VGPR staging),
// three k-tiles in flight behind a COUNTED s_waitcnt vmcnt and one raw s_barrier per k-tile.  LDS-DMA writes
// 1 KiB per wave-instruction linearly (lane i -> base + 16 i), so the images cannot be padded; bank conflicts
// are removed by XOR swizzles applied to the SOURCE address (which 16-B chunk a lane fetches):
//   K-major operand  : image [row][32 k] (64-B rows); chunk c of row r sits at position c ^ 2*((r>>2)&1);
//                      fragments by ds_read_b128.
//   m-major operand  : image [32 k][ROWS m] exactly as stored in HBM; chunk c of k-row kr sits at
//                      c ^ 2*f(kr) with f = (kr&3)|4*((kr>>3)&1) for 256-B rows, ((kr>>1)&1)|2*((kr>>3)&1)
//                      for 128-B rows; fragments by two ds_read_b64_tr_b16 (each 32-lane half then touches
//                      eight different 32-B slots of the 256-B bank row).
template <int ROWS> __device__ __forceinline__ int mmajor_f(int kr) {
  if constexpr (ROWS == 128) return (kr & 3) | (((kr >> 3) & 1) << 2);
  else return ((kr >> 1) & 1) | (((kr >> 3) & 1) << 1);
}

typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned u32x2;

// The main loop below is scheduled by hand: LDS fragment reads, MFMAs and the counted waits are `asm volatile`, so
// hipcc neither reorders them nor adds its own conservative s_waitcnt (a compiler-visible ds_read next to an asm one
// made it drain lgkmcnt to 0 every k-tile; the ds_read_tr builtin made it drain vmcnt, i.e. the LDS-DMA ring).
template <int OFF> __device__ __forceinline__ u32x4 lds_read_b128(unsigned addr) {
  u32x4 v;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF) : "memory");
  return v;
}
// 16x16x32 fragment half through the transposing read: 4 consecutive k of one m-column per lane (EXEC must be full)
template <int OFF> __device__ __forceinline__ u32x2 lds_read_tr(unsigned addr) {
  u32x2 v;
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF) : "memory");
  return v;
}
__device__ __forceinline__ void mfma_bf16_asm(f32x4& acc, const u32x4& x, const u32x4& y) {
  asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(acc) : "v"(x), "v"(y));
}
// at most g groups of LPS LDS-DMA instructions may stay in flight
template <int LPS> __device__ __forceinline__ void wait_groups(int g) {
  switch (g) {
    case 0: wait_vmcnt<0>(); break;
    case 1: wait_vmcnt<LPS>(); break;
    case 2: wait_vmcnt<2 * LPS>(); break;
    default: wait_vmcnt<3 * LPS>(); break;
  }
}

// E: bf16_t, or char for K-major fp8 (the K-major image is byte-wise: a 64-byte row is 32 bf16 or 64 e4m3 values of k)
template <int ROWS, bool KMAJOR, int NWAVES = 4, int NFRAG = ROWS / 32, typename E = bf16_t>
struct GldsOperand {
  static_assert(KMAJOR || sizeof(E) == 2, "the transposing LDS read is a 16-bit one");
  static constexpr int L = ROWS / (16 * NWAVES);   // LDS-DMA instructions per wave per stage
  static constexpr int BYTES = ROWS * 64;          // one stage of this operand
  static constexpr int NF = NFRAG;                 // 16-row fragments per wave (2 x 2 waves: the wave owns ROWS/2 rows)
  static constexpr int RPF = KMAJOR ? 1 : 2;       // LDS read instructions per fragment
  const E* src[L];
  long kstep;                                      // elements to advance per k-tile
  unsigned foff[KMAJOR ? 1 : NF];                  // per-lane LDS byte offsets of the fragments inside a stage
  __device__ __forceinline__ void init(const E* base, long ld, int row0, int nrows, int wave, int lane, int wrow0) {
    if constexpr (KMAJOR) {
      const int lrow = lane >> 2, lpos = lane & 3;
      const int lchunk = lpos ^ (((lrow >> 2) & 1) << 1);
#pragma unroll
      for (int i = 0; i < L; ++i) {
        int r = row0 + (wave * L + i) * 16 + lrow;
        r = r < nrows ? r : nrows - 1;             // rows past the edge are never stored
        src[i] = base + (long)r * ld + lchunk * (16 / (int)sizeof(E));
      }
      kstep = 64 / (int)sizeof(E);
      const int fr = lane & 15, fc = lane >> 4;    // fragment i sits 16 rows = 1024 B further: an immediate offset
      foff[0] = (unsigned)((wrow0 + fr) * 64 + ((fc ^ (((fr >> 2) & 1) << 1)) * 16));
    } else {
      constexpr int CPR = ROWS / 8, KR = 64 / CPR;  // chunks per k-row, k-rows per wave-instruction
      const int kl = lane / CPR, pos = lane % CPR;
#pragma unroll
      for (int i = 0; i < L; ++i) {
        const int kr = (wave * L + i) * KR + kl;
        int m = row0 + ((pos ^ (mmajor_f<ROWS>(kr) << 1)) * 8);
        m = m + 8 <= nrows ? m : nrows - 8;
        src[i] = base + (long)kr * ld + m;
      }
      kstep = 32 * ld;
      // two reads per fragment: k-rows kr0 = 8 g + q4 and kr0 + 4 (same swizzle term: f(kr0 + 4) == f(kr0)), so the
      // second read is the first plus 4 k-rows = 8 * ROWS bytes, an immediate
      const int g = lane >> 4, q4 = (lane & 15) >> 2, pp = lane & 3;
      const int kr0 = 8 * g + q4;
#pragma unroll
      for (int i = 0; i < NF; ++i) {
        const int chunk = ((wrow0 + i * 16) >> 3) + (pp >> 1);
        foff[i] = (unsigned)(kr0 * (ROWS * 2) + ((chunk ^ (mmajor_f<ROWS>(kr0) << 1)) * 16) + (pp & 1) * 8);
      }
    }
  }
  // LDS-DMA instruction i of k-tile kt into the stage at `stage`
  __device__ __forceinline__ void issue1(int i, int kt, char* stage, int wave) const {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src[i] + kt * kstep),
                                     (__attribute__((address_space(3))) void*)(stage + (wave * L + i) * 1024), 16, 0, 0);
  }
  // read instruction r (0 .. NF*RPF-1) of a stage whose byte address is sbase + SOFF; results land in fr[]
  template <int R, int SOFF>
  __device__ __forceinline__ void read1(unsigned sbase, u32x4 (&fr)[NF]) const {
    if constexpr (KMAJOR) {
      fr[R] = lds_read_b128<SOFF + R * 1024>(sbase + foff[0]);
    } else {
      constexpr int i = R >> 1;
      const u32x2 h = lds_read_tr<SOFF + (R & 1) * 8 * ROWS>(sbase + foff[i]);
      if constexpr ((R & 1) == 0) { fr[i][0] = h[0]; fr[i][1] = h[1]; }
      else { fr[i][2] = h[0]; fr[i][3] = h[1]; }
    }
  }
};

// The workgroup's share of an LDS-DMA ring kernel: its output tile (bm0, bn0) and its k-tiles [kt0, kt0 + nt) of BK -- block
// bid / tiles takes the bid / tiles'th of p.splits equal K ranges.  Textual for the same reason as gemm_glds_loop.h.
#define KLAB_GLDS_WORK(BK)                                                              \
  const int tiles = ((p.M + BM - 1) / BM) * ((p.N + BN - 1) / BN);                      \
  const int tile = bid % tiles, split = bid / tiles;                                    \
  int bm0, bn0;                                                                         \
  tile_of_block(p, BM, BN, tile, bm0, bn0);                                             \
  const int nt_all = p.K / (BK);                                                        \
  const int per = (nt_all + p.splits - 1) / p.splits;                                   \
  const int kt0 = split * per, kt1 = (kt0 + per < nt_all) ? kt0 + per : nt_all;         \
  const int nt = kt1 - kt0;                                                             \
  if (nt <= 0) return;

// 4 waves (2 x 2) on a BM x BN tile, any operand layout; ATOMIC: split-K partial sums added to C with float atomics.
// MAY_STORE (with ATOMIC; the grouped kernel's store members): p.accumulate == 0 writes the tile with plain stores from the same
// accumulator layout instead; such a product must not be split along K (p.splits == 1), C is never read.
template <int BM, int BN, bool AK, bool BKM, bool ATOMIC, bool MAY_STORE = false>
__device__ __forceinline__ void gemm_glds_body(const GemmP& p, const int bid = blockIdx.x) {
  typedef bf16_t T;
  constexpr int WTM = BM / 2, WTN = BN / 2, MI = WTM / 16, NI = WTN / 16;
  typedef GldsOperand<BM, AK> OA;
  typedef GldsOperand<BN, BKM> OB;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = (wave >> 1) * WTM, wn = (wave & 1) * WTN;
  KLAB_GLDS_WORK(32)

  OA oa; OB ob;
  oa.init(reinterpret_cast<const T*>(p.A), p.lda, bm0, p.M, wave, lane, wm);
  ob.init(reinterpret_cast<const T*>(p.B), p.ldb, bn0, p.N, wave, lane, wn);
  // operands swapped (the B tile as the MFMA "A" operand: a lane's four accumulator registers are four consecutive n), except
  // for ATOMIC, whose float atomics then cover 16 consecutive n per wave-instruction
#define KLAB_RING_MMA(ACC, A, B) if constexpr (ATOMIC) mfma_bf16_asm(ACC, A, B); else mfma_bf16_asm(ACC, B, A);
#define KLAB_RING_TWO_BASES 0
#define KLAB_RING_DRAIN4 1
#include "gemm_glds_loop.h"
  float alpha = p.alpha;
  if (p.alpha_dev) alpha *= p.alpha_dev[0];
  if constexpr (ATOMIC) {
    float* Cf = reinterpret_cast<float*>(p.C);
    bool store = false;
    if constexpr (MAY_STORE) store = !p.accumulate;  // workgroup-uniform
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int j = 0; j < NI; ++j) {
        const int n = bn0 + wn + j * 16 + (lane & 15);
        if (n >= p.N) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int m = bm0 + wm + i * 16 + (lane >> 4) * 4 + r;
          if (m >= p.M) continue;
          if (store) Cf[(long)m * p.ldc + n] = acc[i][j][r] * alpha;
          else atomicAdd(Cf + (long)m * p.ldc + n, acc[i][j][r] * alpha);
        }
      }
  } else {
    __syncthreads();  // all LDS-DMA retired (vmcnt(0) above) and all fragment reads done: LDS is free for the epilogue
    staged_epilogue<T, BM, BN, MI, NI>(p, acc, alpha, smem, bm0, bn0, wm, wn, tid, lane);
  }
}
// 8 waves (4 x 2 of 64 x 64) on a 256 x 128 tile, A K-major; the 96 KB ring needs two LDS base registers
template <bool BKM>
__device__ __forceinline__ void gemm_glds_w8_body(const GemmP& p, const int bid = blockIdx.x) {
  typedef bf16_t T;
  constexpr int BM = 256, BN = 128;
  constexpr int WTM = BM / 4, WTN = BN / 2, MI = WTM / 16, NI = WTN / 16;
  typedef GldsOperand<BM, true, 8, MI> OA;
  typedef GldsOperand<BN, BKM, 8, NI> OB;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = (wave >> 1) * WTM, wn = (wave & 1) * WTN;  // wave 0..7
  KLAB_GLDS_WORK(32)

  OA oa; OB ob;
  oa.init(reinterpret_cast<const T*>(p.A), p.lda, bm0, p.M, wave, lane, wm);
  ob.init(reinterpret_cast<const T*>(p.B), p.ldb, bn0, p.N, wave, lane, wn);
#define KLAB_RING_MMA(ACC, A, B) mfma_bf16_asm(ACC, B, A);
#define KLAB_RING_TWO_BASES 1
#define KLAB_RING_DRAIN4 0
#include "gemm_glds_loop.h"
  float alpha = p.alpha;
  if (p.alpha_dev) alpha *= p.alpha_dev[0];
  __syncthreads();  // all LDS-DMA retired (vmcnt(0) above) and all fragment reads done: LDS is free for the epilogue
  staged_epilogue<T, BM, BN, MI, NI, 512>(p, acc, alpha, smem, bm0, bn0, wm, wn, tid, lane);
}
template <bool BKM>
__global__ __launch_bounds__(512) void gemm_glds_w8_kernel(GemmP p) { gemm_glds_w8_body<BKM>(p); }

template <int BM, int BN, bool AK, bool BKM, bool ATOMIC>
__global__ __launch_bounds__(256) void gemm_glds_kernel(GemmP p) { gemm_glds_body<BM, BN, AK, BKM, ATOMIC>(p); }

// Grouped launch: up to 8 independent split-K weight-gradient GEMMs (both operands m-major, f32 atomic accumulation) in ONE
// grid.  A layer's 4-7 weight gradients are 2-9 GFLOP each: launched one by one on the side stream each of them under-fills
// the chip and pays its own launch; together they are one ~30 GFLOP kernel whose small members fill the big ones' tails.
// A member with accumulate == 0 (a store member) is never split along K (splits == 1) and writes its tiles with plain stores: C
// needs no clearing first.  A computed -0.0 then stays -0.0 where 0 + -0.0 gave +0.0; nothing downstream tells them apart (Adam
// squares or scales the value, torch.equal takes them as equal).
struct GroupEntry { const void* A; long lda; const void* B; long ldb; float* C; long ldc; int M, N, K, splits, start; float alpha; int accumulate; };
struct GroupP { GroupEntry e[8]; int n; };
template <int BN>
__global__ __launch_bounds__(256) void gemm_glds_grouped_tn_kernel(GroupP g) {
  int k = 0;
#pragma unroll
  for (int i = 1; i < 8; ++i)
    if (i < g.n && (int)blockIdx.x >= g.e[i].start) k = i;
  const GroupEntry& e = g.e[k];
  GemmP p;
  p.M = e.M; p.N = e.N; p.K = e.K;
  p.A = e.A; p.lda = e.lda; p.a_kmajor = 0; p.B = e.B; p.ldb = e.ldb; p.b_kmajor = 0;
  p.C = e.C; p.ldc = e.ldc; p.c_f32 = 1; p.accumulate = e.accumulate;
  p.alpha = e.alpha; p.alpha_dev = nullptr; p.bias = nullptr; p.act = 0;
  p.aux = nullptr; p.ldaux = 0; p.aux_mode = 0; p.aux_scale = 1.f; p.residual = nullptr; p.ldr = 0; p.r_f32 = 1;
  p.drop_p = 0.f; p.seed = nullptr; p.tag = 0; p.splits = e.accumulate ? e.splits : 1; p.epi = 0;
  // (measured: members whose K is not split adding their tile with staged, coalesced read-modify-writes instead of 16 K float
  // atomics per tile -- 0.082 vs 0.079 ms per launch, no change in the step: the atomics are not what bounds this kernel)
  gemm_glds_body<128, BN, false, false, true, true>(p, (int)blockIdx.x - e.start);
}

// One workgroup = 4 waves (2x2) computing a BM x BN tile over k-tiles [kt0, kt1).
// ATOMIC: split-K partial sums are added to a pre-zeroed / accumulating f32 C with float atomics; the
// MFMA operands are then NOT swapped so that each atomic wave-instruction covers 16 consecutive n (64 B).
template <typename T, int BM, int BN, bool AK, bool BKM, bool ATOMIC>
__device__ __forceinline__ void gemm_body(const GemmP& p) {
  constexpr int BK = MmaTraits<T>::BK;
  constexpr int WTM = BM / 2, WTN = BN / 2;  // wave tile (2x2 waves)
  constexpr int MI = WTM / 16, NI = WTN / 16;
  constexpr int ABYTES = TileBytes<T, BM, AK>::value, BBYTES = TileBytes<T, BN, BKM>::value;
  constexpr int STAGE = ABYTES + BBYTES;  // one pipeline stage: A tile then B tile
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = (wave >> 1) * WTM, wn = (wave & 1) * WTN;
  const int tiles_m = (p.M + BM - 1) / BM, tiles_n = (p.N + BN - 1) / BN;
  const int tiles = tiles_m * tiles_n;
  const int tile = blockIdx.x % tiles, split = blockIdx.x / tiles;
  int bm0, bn0;
  tile_of_block(p, BM, BN, tile, bm0, bn0);

  const T* A = reinterpret_cast<const T*>(p.A);
  const T* B = reinterpret_cast<const T*>(p.B);
  Stager<T, BM, AK> sa;
  Stager<T, BN, BKM> sb;

  f32x4 acc[MI][NI];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nt_all = (p.K + BK - 1) / BK;
  const int per = (nt_all + p.splits - 1) / p.splits;
  const int kt0 = split * per, kt1 = (kt0 + per < nt_all) ? kt0 + per : nt_all;
  const int nt = kt1 - kt0;
  if (nt <= 0) return;
  sa.load(A, p.lda, bm0, kt0 * BK, p.M, p.K, tid);
  sb.load(B, p.ldb, bn0, kt0 * BK, p.N, p.K, tid);
  sa.store(smem, tid);
  sb.store(smem + ABYTES, tid);
  __syncthreads();

  for (int t = 0; t < nt; ++t) {
    const int cur = t & 1;
    if (t + 1 < nt) {
      sa.load(A, p.lda, bm0, (kt0 + t + 1) * BK, p.M, p.K, tid);
      sb.load(B, p.ldb, bn0, (kt0 + t + 1) * BK, p.N, p.K, tid);
    }
    const char* ta = smem + cur * STAGE;
    const char* tb = ta + ABYTES;
    if constexpr (sizeof(T) == 2) {
#pragma unroll
      for (int ks = 0; ks < BK / 32; ++ks) {
        bf16x8 af[MI], bfr[NI];
#pragma unroll
        for (int i = 0; i < MI; ++i) af[i] = load_frag_bf16<BM, AK>(ta, wm + i * 16, ks, lane);
#pragma unroll
        for (int j = 0; j < NI; ++j) bfr[j] = load_frag_bf16<BN, BKM>(tb, wn + j * 16, ks, lane);
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
          for (int j = 0; j < NI; ++j) {
            if constexpr (ATOMIC) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
            else acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[j], af[i], acc[i][j], 0, 0, 0);
          }
      }
    } else {
      const char* la = ta + (wm + (lane & 15)) * ROWB;
      const char* lb = tb + (wn + (lane & 15)) * ROWB;
#pragma unroll
      for (int ks = 0; ks < BK / 4; ++ks) {
        float af[MI], bfr[NI];
        const int koff = (ks * 4 + (lane >> 4)) * 4;
#pragma unroll
        for (int i = 0; i < MI; ++i) af[i] = *reinterpret_cast<const float*>(la + i * 16 * ROWB + koff);
#pragma unroll
        for (int j = 0; j < NI; ++j) bfr[j] = *reinterpret_cast<const float*>(lb + j * 16 * ROWB + koff);
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
          for (int j = 0; j < NI; ++j) {
            if constexpr (ATOMIC) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i], bfr[j], acc[i][j], 0, 0, 0);
            else acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(bfr[j], af[i], acc[i][j], 0, 0, 0);
          }
      }
    }
    if (t + 1 < nt) {
      sa.store(smem + (cur ^ 1) * STAGE, tid);
      sb.store(smem + (cur ^ 1) * STAGE + ABYTES, tid);
    }
    __syncthreads();
  }

  float alpha = p.alpha;
  if (p.alpha_dev) alpha *= p.alpha_dev[0];
  if constexpr (ATOMIC) {
    // lane owns n = ... + (lane&15), m = ... + (lane>>4)*4 + r
    float* Cf = reinterpret_cast<float*>(p.C);
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int j = 0; j < NI; ++j) {
        const int n = bn0 + wn + j * 16 + (lane & 15);
        if (n >= p.N) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int m = bm0 + wm + i * 16 + (lane >> 4) * 4 + r;
          if (m < p.M) atomicAdd(Cf + (long)m * p.ldc + n, acc[i][j][r] * alpha);
        }
      }
  } else {
    staged_epilogue<T, BM, BN, MI, NI>(p, acc, alpha, smem, bm0, bn0, wm, wn, tid, lane);
  }
}

template <typename T, int BM, int BN, bool AK, bool BKM, bool ATOMIC>
__global__ __launch_bounds__(256) void gemm_kernel(GemmP p) { gemm_body<T, BM, BN, AK, BKM, ATOMIC>(p); }
// the LM-head logits GEMM under its own symbol, so that profiles and the in-process probe
// (klab_engine_probe_*) can be matched kernel for kernel
template <typename T>
__global__ __launch_bounds__(256) void klab_lmhead_gemm(GemmP p) {
  if constexpr (sizeof(T) == 2) gemm_glds_body<128, 128, true, true, false>(p);
  else gemm_body<T, 128, 128, true, true, false>(p);
}

template <typename K>
static int launch_kernel(K kern, const GemmP& p, int BM, int BN, size_t lds, hipStream_t s) {
  {
    const int rc = ensure_dyn_lds(reinterpret_cast<const void*>(kern), lds);
    if (rc) return rc;
  }
  const long tm = (p.M + BM - 1) / BM, tn = (p.N + BN - 1) / BN;
  probed_launch(kern, dim3((unsigned)(tm * tn * p.splits)), dim3(256), lds, s, p);
  KLAB_LAUNCH_CHECK();
  return KLAB_OK;
}

template <typename T, int BM, int BN, bool AK, bool BKM>
static int launch_gemm(const GemmP& p, bool atomic, hipStream_t s) {
  size_t lds = 2 * (size_t)(TileBytes<T, BM, AK>::value + TileBytes<T, BN, BKM>::value);
  const size_t epi = (size_t)epilogue_lds_bytes<BM, BN>(p.c_f32 || sizeof(T) == 4);
  if (!atomic && epi > lds) lds = epi;
  if (atomic) return launch_kernel(gemm_kernel<T, BM, BN, AK, BKM, true>, p, BM, BN, lds, s);
  return launch_kernel(gemm_kernel<T, BM, BN, AK, BKM, false>, p, BM, BN, lds, s);
}

template <int BM, int BN, bool AK, bool BKM>
static int launch_glds(const GemmP& p, bool atomic, hipStream_t s) {
  const int nt = (p.K / 32 + p.splits - 1) / p.splits;
  size_t lds = (size_t)(nt < KLAB_GLDS_STAGES ? nt : KLAB_GLDS_STAGES) * (BM + BN) * 64;  // short K: fewer stages => more workgroups per CU
  if (!atomic) {
    const size_t epi = (size_t)epilogue_lds_bytes<BM, BN>(p.c_f32);
    if (epi > lds) lds = epi;
    return launch_kernel(gemm_glds_kernel<BM, BN, AK, BKM, false>, p, BM, BN, lds, s);
  }
  return launch_kernel(gemm_glds_kernel<BM, BN, AK, BKM, true>, p, BM, BN, lds, s);
}

template <typename T, int BM, int BN>
static int dispatch_layout(const GemmP& p, bool atomic, hipStream_t s) {
  if constexpr (sizeof(T) == 2) {
    // LDS-DMA path: whole 32-deep k-tiles, and m-major operands need a full 8-element chunk inside the matrix
    const bool ok = (p.K % 32) == 0 && p.K >= 32 && (p.a_kmajor || p.M >= 8) && (p.b_kmajor || p.N >= 8);
    if (ok) {
      if (p.a_kmajor && p.b_kmajor) return launch_glds<BM, BN, true, true>(p, atomic, s);
      if (p.a_kmajor && !p.b_kmajor) return launch_glds<BM, BN, true, false>(p, atomic, s);
      if (!p.a_kmajor && p.b_kmajor) return launch_glds<BM, BN, false, true>(p, atomic, s);
      return launch_glds<BM, BN, false, false>(p, atomic, s);
    }
  }
  if (p.a_kmajor && p.b_kmajor) return launch_gemm<T, BM, BN, true, true>(p, atomic, s);
  if (p.a_kmajor && !p.b_kmajor) return launch_gemm<T, BM, BN, true, false>(p, atomic, s);
  if (!p.a_kmajor && p.b_kmajor) return launch_gemm<T, BM, BN, false, true>(p, atomic, s);
  return launch_gemm<T, BM, BN, false, false>(p, atomic, s);
}

// tile / split-K choice: the largest tile that still gives about one workgroup per CU; when even the
// smallest does not and the caller allows atomic accumulation, split K until the chip is covered.
int mm8p_try(const GemmP& pin, bool atomic_ok, int force, hipStream_t s);  // mm8p.hip: 256 x 256 tiles, eight waves, BK = 64
int mmf8_try(const GemmP& pin, const float* sa, const float* sb, long sb_stride, int force, hipStream_t s);  // mmf8.hip: block-scaled fp8 MFMA
int mm8p_grouped_try(const klab_gemm_args* list, int n, bool large_tiles, hipStream_t s);  // mm8p.hip: a layer's weight gradients on 256 x 256 tiles

template <typename T>
static int dispatch_tile(GemmP& p, bool atomic_ok, hipStream_t s, int p8_force = 0) {
  auto tiles = [&](int bm, int bn) { return (long)((p.M + bm - 1) / bm) * ((p.N + bn - 1) / bn); };
  if constexpr (sizeof(T) == 2) {
    if (p8_force >= 0) {  // the large-tile kernel first: it declines (KLAB_ERR_UNSUPPORTED) what it is not built for
      const int rc = mm8p_try(p, atomic_ok, p8_force, s);
      if (rc != KLAB_ERR_UNSUPPORTED) return rc;
    }
  }
  const int BK = MmaTraits<T>::BK;
  const int nt = (p.K + BK - 1) / BK;
  p.splits = 1;
  if (atomic_ok && nt >= 256 && p.M >= 128 && p.N >= 64 && tiles(128, 64) < 1024) {
    // very long K over few tiles (LM-head dgrad: K = vocabulary): one workgroup per CU streams its operands from HBM
    // with too little in flight; split K so that ~4 workgroups share a CU.  128x128 tiles when N allows: the streamed
    // operand (263 MB of dlogits) is re-read once per column tile, i.e. 4x instead of 8x for N = 512.
    const bool wide = p.N >= 128;
    const long t = wide ? tiles(128, 128) : tiles(128, 64);
    long sp = (1024 + t - 1) / t;
    if (sp > nt / 64) sp = nt / 64;
    if (sp > 16) sp = 16;
    if (sp >= 2) {
      p.splits = (int)sp;
      return wide ? dispatch_layout<T, 128, 128>(p, true, s) : dispatch_layout<T, 128, 64>(p, true, s);
    }
  }
  if constexpr (sizeof(T) == 2) {
    // 256 x 128 tiles on eight waves (4 x 2 of 64 x 64; 85 FLOP per operand byte instead of 64; one workgroup per CU).  Measured
    // per shape (tools/gemm_bench.py): it wins where 128 x 128 tiles need a second,
    // poorly filled round of workgroups and the big tiles fit in ONE round (T5-large wo forward 75.7 -> 63.0 us, wi / qkv dgrad
    // 64 -> 56 / 52 -> 47 us), ties or loses everywhere else (several rounds of one-per-CU workgroups expose every epilogue)
    const bool w8_fits = p.a_kmajor && (p.K % 32) == 0 && p.K >= 128 && p.M >= 256 && p.N >= 128 && (p.b_kmajor || p.N >= 8);
    // (inside the configs[1] step, K = 512, the same rule measured 0.7 % SLOWER -- 6.40 vs 6.35 ms -- hence K >= 1024; configs[4] +0.6 %)
    if (w8_fits && p.K >= 1024 && tiles(128, 128) > 256 && tiles(256, 128) <= 256) {
      const int nt = p.K / 32;
      size_t lds = (size_t)(nt < KLAB_GLDS_STAGES ? nt : KLAB_GLDS_STAGES) * (256 + 128) * 64;
      const size_t epi = (size_t)epilogue_lds_bytes<256, 128>(p.c_f32);
      if (epi > lds) lds = epi;
      const void* kern = p.b_kmajor ? reinterpret_cast<const void*>(gemm_glds_w8_kernel<true>) : reinterpret_cast<const void*>(gemm_glds_w8_kernel<false>);
      const int rc = ensure_dyn_lds(kern, lds);
      if (rc) return rc;
      if (p.b_kmajor) probed_launch(gemm_glds_w8_kernel<true>, dim3((unsigned)tiles(256, 128)), dim3(512), lds, s, p);
      else probed_launch(gemm_glds_w8_kernel<false>, dim3((unsigned)tiles(256, 128)), dim3(512), lds, s, p);
      KLAB_LAUNCH_CHECK();
      return KLAB_OK;
    }
  }
  // a grid of about one workgroup per CU or more.  224, not 240: the T5-small encoder's M = 3712 gives 29 x 8 = 232 tiles of
  // 128 x 64, which measured 0.4 % faster per step than the 464 tiles of 64 x 64 the higher threshold chose (same box, 3 rounds:
  // 6.135 / 6.139 / 6.167 vs 6.173 / 6.159 / 6.179 ms).
  constexpr int TILE_MIN = 224;
  if (tiles(128, 128) >= TILE_MIN) return dispatch_layout<T, 128, 128>(p, false, s);
  if (tiles(128, 64) >= TILE_MIN) return dispatch_layout<T, 128, 64>(p, false, s);
  if (atomic_ok && nt >= 16) {
    const bool big = p.M >= 128 && p.N >= 64;
    const long t = big ? tiles(128, 64) : tiles(64, 64);
    long sp = (256 + t - 1) / t;
    if (sp > nt / 8) sp = nt / 8;   // at least 8 k-tiles (512 k) per split
    if (sp > 16) sp = 16;
    if (sp >= 2) {
      p.splits = (int)sp;
      return big ? dispatch_layout<T, 128, 64>(p, true, s) : dispatch_layout<T, 64, 64>(p, true, s);
    }
  }
  return dispatch_layout<T, 64, 64>(p, false, s);
}

// ---- fp8 forward GEMM (BASELINE configs[4]: "fp8 MFMA path") -----------------------------------------------------------
// C[M,N] = epilogue(alpha * sa[m] * sb[n] * sum_k A8(m,k) B8(n,k)): both operands K-major OCP e4m3 bytes (gfx950's native
// fp8), one dequantisation scale per ROW of each operand (per token / per output channel; per-tensor scaling is the special
// case of equal entries), fp32 accumulation on v_mfma_f32_16x16x32_fp8_fp8.  The accumulator layout equals the bf16
// kernels', so the whole epilogue family (bias, relu, gelu, dropout, residual, bf16 / f32 output) is shared with them.
// Register-staged, double-buffered: 128-byte k-tiles (128 fp8 values), rows padded to 144 B in LDS, ds_read_b64 fragments.
struct Fp8Scales { const float* sa; const float* sb; long sb_stride; };

template <int BM, int BN>
__global__ __launch_bounds__(256) void gemm_fp8_kernel(GemmP p, Fp8Scales sc) {
  constexpr int BK = 128;
  constexpr int WTM = BM / 2, WTN = BN / 2, MI = WTM / 16, NI = WTN / 16;
  constexpr int ABYTES = BM * ROWB, BBYTES = BN * ROWB, STAGE = ABYTES + BBYTES;
  constexpr int ACH = BM * 8 / 256, BCH = BN * 8 / 256;  // 16-byte chunks per thread
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = (wave >> 1) * WTM, wn = (wave & 1) * WTN;
  int bm0, bn0;
  tile_of_block(p, BM, BN, blockIdx.x, bm0, bn0);
  const char* A = reinterpret_cast<const char*>(p.A);
  const char* B = reinterpret_cast<const char*>(p.B);
  f32x4 va[ACH], vb[BCH];
  auto load = [&](int k0) {
#pragma unroll
    for (int c = 0; c < ACH; ++c) {
      const int ch = tid + c * 256, r = ch >> 3, kc = ch & 7;
      const int gr = bm0 + r, gk = k0 + kc * 16;
      const bool ok = gr < p.M && gk < p.K;
      f32x4 z = *reinterpret_cast<const f32x4*>(A + (long)(gr < p.M ? gr : p.M - 1) * p.lda + (gk < p.K ? gk : p.K - 16));
      if (!ok) z = f32x4{0.f, 0.f, 0.f, 0.f};  // all-zero bytes = fp8 +0
      va[c] = z;
    }
#pragma unroll
    for (int c = 0; c < BCH; ++c) {
      const int ch = tid + c * 256, r = ch >> 3, kc = ch & 7;
      const int gr = bn0 + r, gk = k0 + kc * 16;
      const bool ok = gr < p.N && gk < p.K;
      f32x4 z = *reinterpret_cast<const f32x4*>(B + (long)(gr < p.N ? gr : p.N - 1) * p.ldb + (gk < p.K ? gk : p.K - 16));
      if (!ok) z = f32x4{0.f, 0.f, 0.f, 0.f};
      vb[c] = z;
    }
  };
  auto store = [&](char* st) {
#pragma unroll
    for (int c = 0; c < ACH; ++c) { const int ch = tid + c * 256; *reinterpret_cast<f32x4*>(st + (ch >> 3) * ROWB + (ch & 7) * 16) = va[c]; }
#pragma unroll
    for (int c = 0; c < BCH; ++c) { const int ch = tid + c * 256; *reinterpret_cast<f32x4*>(st + ABYTES + (ch >> 3) * ROWB + (ch & 7) * 16) = vb[c]; }
  };
  f32x4 acc[MI][NI];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int nt = (p.K + BK - 1) / BK;
  load(0);
  store(smem);
  __syncthreads();
  for (int t = 0; t < nt; ++t) {
    const int cur = t & 1;
    if (t + 1 < nt) load((t + 1) * BK);
    const char* ta = smem + cur * STAGE + (wm + (lane & 15)) * ROWB + (lane >> 4) * 8;
    const char* tb = smem + cur * STAGE + ABYTES + (wn + (lane & 15)) * ROWB + (lane >> 4) * 8;
#pragma unroll
    for (int ks = 0; ks < BK / 32; ++ks) {
      long af[MI], bfr[NI];
#pragma unroll
      for (int i = 0; i < MI; ++i) af[i] = *reinterpret_cast<const long*>(ta + i * 16 * ROWB + ks * 32);
#pragma unroll
      for (int j = 0; j < NI; ++j) bfr[j] = *reinterpret_cast<const long*>(tb + j * 16 * ROWB + ks * 32);
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(bfr[j], af[i], acc[i][j], 0, 0, 0);
    }
    if (t + 1 < nt) store(smem + (cur ^ 1) * STAGE);
    __syncthreads();
  }
  // dequantise: lane owns m = ... + (lane & 15), n = ... + (lane >> 4) * 4 + r
#pragma unroll
  for (int i = 0; i < MI; ++i) {
    const int m = bm0 + wm + i * 16 + (lane & 15);
    const float sam = sc.sa[m < p.M ? m : p.M - 1];
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      const int n0 = bn0 + wn + j * 16 + (lane >> 4) * 4;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = n0 + r < p.N ? n0 + r : p.N - 1;
        acc[i][j][r] *= sam * sc.sb[(long)n * sc.sb_stride];
      }
    }
  }
  float alpha = p.alpha;
  if (p.alpha_dev) alpha *= p.alpha_dev[0];
  staged_epilogue<bf16_t, BM, BN, MI, NI>(p, acc, alpha, smem, bm0, bn0, wm, wn, tid, lane);
}


// ---- fp8 on the LDS-DMA ring ------------------------------------------------------------------------------------------------
// The K-major LDS image of the bf16 kernels is byte-wise: 64-byte rows, 16-byte chunks XOR-swizzled by the source address.  With
// e4m3 operands a row holds 64 k values; a lane's ds_read_b128 returns 16 consecutive k of its row (chunk c = lane >> 4), which
// feed TWO v_mfma_f32_16x16x32_fp8_fp8: the low 8 bytes of both operands, then the high 8 bytes.  The first instruction therefore
// contracts k in {16 g + 0..7}, the second k in {16 g + 8..15} (g = 0..3): together all 64, each once, and since A and B use the
// same assignment the sum is the dot product.  Same ring, same waits, same hand schedule as gemm_glds_body; half the L2 -> LDS
// bytes per FLOP, which is what bounds these products.
// both halves in ONE asm statement: the compiler sees a single use of the two 128-bit registers and cannot place a copy of an
// asm-loaded (not yet landed) register between the LDS read and its wait
__device__ __forceinline__ void mfma_fp8_asm2(f32x4& acc, const u32x4& x, const u32x4& y) {
  asm volatile("v_mfma_f32_16x16x32_fp8_fp8 %0, %1, %2, %0\n\tv_mfma_f32_16x16x32_fp8_fp8 %0, %3, %4, %0"
               : "+v"(acc)
               : "v"(__builtin_shufflevector(x, x, 0, 1)), "v"(__builtin_shufflevector(y, y, 0, 1)), "v"(__builtin_shufflevector(x, x, 2, 3)),
                 "v"(__builtin_shufflevector(y, y, 2, 3)));
}

template <int BM, int BN>
__device__ __forceinline__ void gemm_glds_fp8_body(const GemmP& p, const Fp8Scales& sc, const int bid = blockIdx.x) {
  typedef bf16_t T;  // output / epilogue element type
  constexpr int BK = 64;  // a k-tile is still 64 BYTES per row: 64 e4m3 values
  constexpr int WTM = BM / 2, WTN = BN / 2, MI = WTM / 16, NI = WTN / 16;
  typedef GldsOperand<BM, true, 4, BM / 32, char> OA;
  typedef GldsOperand<BN, true, 4, BN / 32, char> OB;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = (wave >> 1) * WTM, wn = (wave & 1) * WTN;
  KLAB_GLDS_WORK(BK)

  OA oa; OB ob;
  oa.init(reinterpret_cast<const char*>(p.A), p.lda, bm0, p.M, wave, lane, wm);
  ob.init(reinterpret_cast<const char*>(p.B), p.ldb, bn0, p.N, wave, lane, wn);
#define KLAB_RING_MMA(ACC, A, B) mfma_fp8_asm2(ACC, B, A);
#define KLAB_RING_TWO_BASES 0
#define KLAB_RING_DRAIN4 0
#include "gemm_glds_loop.h"
  float alpha = p.alpha;
  if (p.alpha_dev) alpha *= p.alpha_dev[0];
  // dequantise: lane owns m = ... + (lane & 15), n = ... + (lane >> 4) * 4 + r  (the bf16 kernels' accumulator layout)
#pragma unroll
  for (int i = 0; i < MI; ++i) {
    const int m = bm0 + wm + i * 16 + (lane & 15);
    const float sam = sc.sa[m < p.M ? m : p.M - 1];
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      const int n0 = bn0 + wn + j * 16 + (lane >> 4) * 4;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = n0 + r < p.N ? n0 + r : p.N - 1;
        acc[i][j][r] *= sam * sc.sb[(long)n * sc.sb_stride];
      }
    }
  }
  __syncthreads();  // all LDS-DMA retired (vmcnt(0) above) and all fragment reads done: LDS is free for the epilogue
  staged_epilogue<T, BM, BN, MI, NI>(p, acc, alpha, smem, bm0, bn0, wm, wn, tid, lane);
}
template <int BM, int BN>
__global__ __launch_bounds__(256) void gemm_glds_fp8_kernel(GemmP p, Fp8Scales sc) { gemm_glds_fp8_body<BM, BN>(p, sc); }

__device__ __forceinline__ uint32_t pack4_fp8(float a, float b, float c, float d) {
  int w = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, w, true);
  return (uint32_t)w;
}
// one wave per row: amax -> scale = amax / 448 (e4m3 max), values / scale -> fp8 (round to nearest even, clamped)
__device__ __forceinline__ void quant_row_fp8(const bf16_t* __restrict__ src, int K, uint8_t* __restrict__ dst, float* __restrict__ scale, int lane) {
  constexpr int MAXV = 8;  // K <= 64 lanes * 8 values * MAXV = 4096
  bf16x8 v[MAXV];
  float amax = 0.f;
#pragma unroll
  for (int u = 0; u < MAXV; ++u) {
    const int k = (u * 64 + lane) * 8;
    v[u] = bf16x8{};
    if (k < K) {
      v[u] = *reinterpret_cast<const bf16x8*>(src + k);
#pragma unroll
      for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fabsf((float)v[u][e]));
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
  const float sc = amax > 0.f ? amax * (1.f / 448.f) : 1.f;
  const float inv = 1.f / sc;
  if (lane == 0) *scale = sc;
#pragma unroll
  for (int u = 0; u < MAXV; ++u) {
    const int k = (u * 64 + lane) * 8;
    if (k < K) {
      float f[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) f[e] = fminf(fmaxf((float)v[u][e] * inv, -448.f), 448.f);
      uint2 o2;
      o2.x = pack4_fp8(f[0], f[1], f[2], f[3]);
      o2.y = pack4_fp8(f[4], f[5], f[6], f[7]);
      *reinterpret_cast<uint2*>(dst + k) = o2;
    }
  }
}
__global__ __launch_bounds__(256) void quant_fp8_rows_kernel(const bf16_t* __restrict__ x, long ldx, int M, int K, uint8_t* __restrict__ x8,
                                                             long ld8, float* __restrict__ scale, long scale_stride) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  quant_row_fp8(x + (long)row * ldx, K, x8 + (long)row * ld8, scale + (long)row * scale_stride, threadIdx.x & 63);
}
// every GEMM weight of the compute-dtype arena at once (QuantDesc: multi_tensor.h)
__global__ __launch_bounds__(256) void quant_fp8_arena_kernel(const QuantDesc* __restrict__ dglob, int nd, long total_rows,
                                                              const bf16_t* __restrict__ arena, uint8_t* __restrict__ w8,
                                                              float* __restrict__ wscale) {
  // The tensor table in LDS, workgroups walk the rows grid-stride: a wave's binary search over the table was ~10 dependent global loads
  // (~1.3 us) in front of ONE row's 2-8 KB (the same pattern that held adam_step_kernel at 4.5 TB/s).
  constexpr int MAXD = 1024;
  __shared__ QuantDesc dsh[MAXD];
  const bool in_lds = nd <= MAXD;
  if (in_lds) {
    for (int i = threadIdx.x; i < nd; i += blockDim.x) dsh[i] = dglob[i];
    __syncthreads();
  }
  const QuantDesc* d = in_lds ? dsh : dglob;
  for (long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6); row < total_rows; row += (long)gridDim.x * 4) {
    int lo = 0, hi = nd - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (d[mid].row0 <= row) lo = mid; else hi = mid - 1;
    }
    const long e = d[lo].off + (row - d[lo].row0) * d[lo].K;
    quant_row_fp8(arena + e, (int)d[lo].K, w8 + e, wscale + (e >> 3), threadIdx.x & 63);
  }
}

}  // namespace klab

// klab_gemm_grouped[_tiles]: see include/klab_mm.h.  Members that do not fit the grouped kernel's form are launched one by one.
extern "C" int klab_gemm(const klab_gemm_args* a, void* stream);
extern "C" int klab_gemm_grouped_tiles(const klab_gemm_args* list, int n, int large_tiles, void* stream) {
  using namespace klab;
  if (!list || n < 0) return KLAB_ERR_BADARG;
  {  // large_tiles: the whole list on 256 x 256 tiles without split-K (mm8p.hip) when every member fits that form
    const int rc = mm8p_grouped_try(list, n, large_tiles != 0, (hipStream_t)stream);
    if (rc != KLAB_ERR_UNSUPPORTED) return rc;
  }
  GroupP g;
  g.n = 0;
  int blocks = 0;
  auto fits = [&](const klab_gemm_args* a) {
    return a->dtype == KLAB_BF16 && !a->a_kmajor && !a->b_kmajor && a->c_dtype == KLAB_F32 && a->atomic_ok &&
           !a->bias && !a->act && !a->aux && !a->residual && a->drop_p == 0.f && !a->alpha_dev && a->name_tag == 0 && a->M >= 128 &&
           a->N >= 64 && (a->K % 32) == 0 && a->K >= 512 && !(a->M & 7) && !(a->N & 7) && !(a->lda & 7) && !(a->ldb & 7) &&
           !((uintptr_t)a->A & 15) && !((uintptr_t)a->B & 15) && !((uintptr_t)a->C & 15);
  };
  // 128x128 tiles when every member is at least 128 wide (less operand traffic per flop), else 128x64
  bool wide = true;
  for (int i = 0; i < n; ++i)
    if (fits(&list[i]) && list[i].N < 128) wide = false;
  const int BNr = wide ? 128 : 64;
  auto flush = [&]() -> int {
    if (!g.n) return KLAB_OK;
    const size_t lds = (size_t)KLAB_GLDS_STAGES * (128 + BNr) * 64;
    int rc = ensure_dyn_lds(wide ? reinterpret_cast<const void*>(gemm_glds_grouped_tn_kernel<128>)
                                 : reinterpret_cast<const void*>(gemm_glds_grouped_tn_kernel<64>), lds);
    if (rc) return rc;
    if (wide) probed_launch(gemm_glds_grouped_tn_kernel<128>, dim3((unsigned)blocks), dim3(256), lds, (hipStream_t)stream, g);
    else probed_launch(gemm_glds_grouped_tn_kernel<64>, dim3((unsigned)blocks), dim3(256), lds, (hipStream_t)stream, g);
    KLAB_LAUNCH_CHECK();
    g.n = 0; blocks = 0;
    return KLAB_OK;
  };
  // every workgroup of the group gets about the same number of k-tiles: total work / ~4 workgroups per CU, >= 16 k-tiles
  long work = 0;
  for (int i = 0; i < n; ++i)
    if (fits(&list[i])) work += (long)((list[i].M + 127) / 128) * ((list[i].N + BNr - 1) / BNr) * (list[i].K / 32);
  // round 2 sweep (bench.py, two runs each): target 1024 -> 6.71-6.74 ms/step, 768 -> 6.70-6.72, 384 -> 6.62-6.63, 128 -> 6.64-6.69:
  // fewer, longer workgroups make the grouped kernel itself slower (78 vs 69 us) but leave more of the chip to the main chain
  constexpr int GROUP_TARGET = 384;
  long per_wg = work / (wide ? GROUP_TARGET / 2 : GROUP_TARGET);
  if (per_wg < 16) per_wg = 16;
  for (int i = 0; i < n; ++i) {
    const klab_gemm_args* a = &list[i];
    if (!fits(a)) {
      const int rc = klab_gemm(a, stream);
      if (rc) return rc;
      continue;
    }
    const long t = (long)((a->M + 127) / 128) * ((a->N + BNr - 1) / BNr);
    const int nt = a->K / 32;
    long sp = (nt + per_wg / 2) / per_wg;
    if (sp > nt / 16) sp = nt / 16;
    if (sp > 16) sp = 16;
    if (sp < 1 || !a->accumulate) sp = 1;  // a store member: one workgroup per tile over the whole contraction
    GroupEntry& e = g.e[g.n];
    e.A = a->A; e.lda = a->lda; e.B = a->B; e.ldb = a->ldb; e.C = (float*)a->C; e.ldc = a->ldc;
    e.M = a->M; e.N = a->N; e.K = a->K; e.splits = (int)sp; e.start = blocks; e.alpha = a->alpha; e.accumulate = a->accumulate ? 1 : 0;
    blocks += (int)(t * sp);
    if (++g.n == 8) { const int rc = flush(); if (rc) return rc; }
  }
  return flush();
}
extern "C" int klab_gemm_grouped(const klab_gemm_args* list, int n, void* stream) { return klab_gemm_grouped_tiles(list, n, 0, stream); }

namespace klab {
// klab_gemm_args -> kernel parameters + the epilogue variant (shared by the bf16 / f32 and the fp8 entry points)
static void fill_gemmp(const klab_gemm_args* a, GemmP& p) {
  p.M = a->M; p.N = a->N; p.K = a->K;
  p.A = a->A; p.lda = a->lda; p.a_kmajor = a->a_kmajor;
  p.B = a->B; p.ldb = a->ldb; p.b_kmajor = a->b_kmajor;
  p.C = a->C; p.ldc = a->ldc; p.c_f32 = (a->c_dtype == KLAB_F32); p.accumulate = a->accumulate;
  p.alpha = a->alpha; p.alpha_dev = a->alpha_dev; p.bias = a->bias; p.act = a->act;
  p.aux = a->aux; p.ldaux = a->ldaux; p.aux_mode = a->aux_mode; p.aux_scale = a->aux_scale;
  p.residual = a->residual; p.ldr = a->ldr; p.r_f32 = (a->r_dtype == KLAB_F32);
  p.drop_p = a->drop_p; p.seed = a->seed_dev; p.tag = a->drop_tag;
  p.splits = 1;
  {
    int f = 0;
    if (a->bias) f |= EF_BIAS;
    if (a->act == KLAB_ACT_RELU) f |= EF_RELU;
    if (a->act == KLAB_ACT_GELU) f |= EF_GELU;
    if (a->aux && a->aux_mode == KLAB_AUX_NONZERO) f |= EF_AUXNZ;
    if (a->aux && a->aux_mode == KLAB_AUX_DGELU) f |= EF_DGELU;
    if (a->drop_p > 0.f && a->seed_dev) f |= EF_DROP;
    if (a->residual) f |= EF_RES;
    // copy-out forms (see EF_*_CO): only the exact flag sets that have a variant, and only when every access is a whole
    // aligned 16-byte vector and nothing is accumulated into C
    if (!a->accumulate && a->dtype == KLAB_BF16) {
      if (f == EF_AUXNZ && a->c_dtype == KLAB_BF16 && !(a->N & 7) && !(a->ldc & 7) && !(a->ldaux & 7) && !((uintptr_t)a->aux & 15)) f = EF_AUXNZ_CO;
      if (f == EF_DGELU && a->c_dtype == KLAB_BF16 && !(a->N & 7) && !(a->ldc & 7) && !(a->ldaux & 7) && !((uintptr_t)a->aux & 15)) f = EF_DGELU_CO;
      if ((f == EF_RES || f == (EF_DROP | EF_RES)) && a->c_dtype == KLAB_F32 && a->r_dtype == KLAB_F32 && !(a->N & 3) && !(a->ldc & 3) &&
          !(a->ldr & 3) && !((uintptr_t)a->residual & 15))
        f = (f & ~EF_RES) | EF_RES_CO;
    }
    if ((f & EF_DROP) && (long)a->M * a->N >= (1L << 32)) f = EF_GENERIC;  // dropout indices beyond 32 bits: the general body hashes 64-bit indices
    p.epi = f;  // combinations without a dedicated variant fall into the generic body (switch default)
  }
}
}  // namespace klab

// ---- family probe (measurement only): HIP events around EVERY klab_gemm launch, on the stream it is launched on ------------
// bench.py switches it on for a few untimed steps after the timed region and reports sum(2 M N K) / sum(duration) of the whole
// klab_gemm family (every Linear, dgrad and wgrad of the step) beside the dominant kernel's roofline.  Off: no cost.
namespace klab {
struct GemmProbe {
  std::mutex mu;
  bool on = false;
  std::vector<hipEvent_t> a, b;
  std::vector<double> flops;
  size_t n = 0;
};
static GemmProbe& gemm_probe() { static GemmProbe p; return p; }
}  // namespace klab
static int klab_gemm_impl(const klab_gemm_args* a, void* stream);
extern "C" int klab_gemm_probe_enable(int on) {
  klab::GemmProbe& pr = klab::gemm_probe();
  std::lock_guard<std::mutex> lk(pr.mu);
  if (on && pr.a.empty()) {
    const size_t cap = 8192;
    pr.a.assign(cap, nullptr); pr.b.assign(cap, nullptr); pr.flops.assign(cap, 0.0);
    for (size_t i = 0; i < cap; ++i)
      if (hipEventCreate(&pr.a[i]) != hipSuccess || hipEventCreate(&pr.b[i]) != hipSuccess) return KLAB_ERR_UNSUPPORTED;
  }
  pr.on = on != 0;
  if (on) pr.n = 0;
  return KLAB_OK;
}
extern "C" int klab_gemm_probe_read(int* launches, float* total_ms, double* flops_total) {
  klab::GemmProbe& pr = klab::gemm_probe();
  std::lock_guard<std::mutex> lk(pr.mu);
  float tot = 0.f;
  double fl = 0;
  int cnt = 0;
  for (size_t i = 0; i < pr.n; ++i) {
    if (pr.flops[i] < 0) continue;
    float ms = 0.f;
    const hipError_t er = hipEventElapsedTime(&ms, pr.a[i], pr.b[i]);
    if (er != hipSuccess) { (void)hipGetLastError(); continue; }
    tot += ms;
    fl += pr.flops[i];
    ++cnt;
  }
  if (launches) *launches = cnt;
  if (total_ms) *total_ms = tot;
  if (flops_total) *flops_total = fl;
  return KLAB_OK;
}
extern "C" int klab_gemm(const klab_gemm_args* a, void* stream) {
  klab::GemmProbe& pr = klab::gemm_probe();
  if (!pr.on || !a) return klab_gemm_impl(a, stream);
  size_t slot;
  {
    std::lock_guard<std::mutex> lk(pr.mu);
    if (pr.n >= pr.a.size()) return klab_gemm_impl(a, stream);
    slot = pr.n++;
    pr.flops[slot] = 2.0 * a->M * (double)a->N * a->K;
  }
  klab::tl_launch_probe.a = pr.a[slot];  // the launch this call makes carries the pair as its start / stop events
  klab::tl_launch_probe.b = pr.b[slot];
  const int rc = klab_gemm_impl(a, stream);
  if (klab::tl_launch_probe.a) {  // no tile kernel was launched (empty product, a path outside the family): the slot stays empty
    klab::tl_launch_probe.a = nullptr;
    std::lock_guard<std::mutex> lk(pr.mu);
    pr.flops[slot] = -1.0;
  }
  return rc;
}

namespace klab { int lmhead_areg_try(const GemmP& p, hipStream_t s); }  // lmhead_areg.hip
static int klab_gemm_impl(const klab_gemm_args* a, void* stream) {
  using namespace klab;
  if (!a || !a->A || !a->B || !a->C) return KLAB_ERR_BADARG;
  if (a->M <= 0 || a->N <= 0 || a->K <= 0) return KLAB_OK;
  const int vec = a->dtype == KLAB_BF16 ? 8 : 4;
  // 16-byte vector staging: the contiguous dimension of each operand must be a multiple of `vec`
  if (a->lda % vec || a->ldb % vec) return KLAB_ERR_UNSUPPORTED;
  if (a->a_kmajor ? (a->K % vec) : (a->M % vec)) return KLAB_ERR_UNSUPPORTED;
  if (a->b_kmajor ? (a->K % vec) : (a->N % vec)) return KLAB_ERR_UNSUPPORTED;
  if (((uintptr_t)a->A & 15) || ((uintptr_t)a->B & 15) || ((uintptr_t)a->C & 15)) return KLAB_ERR_UNSUPPORTED;
  if (a->dtype != KLAB_F32 && a->dtype != KLAB_BF16) return KLAB_ERR_BADARG;
  if (a->c_dtype != KLAB_F32 && a->c_dtype != a->dtype) return KLAB_ERR_BADARG;
  GemmP p;
  fill_gemmp(a, p);
  hipStream_t s = (hipStream_t)stream;
  if (a->name_tag == 1 && a->a_kmajor && a->b_kmajor) {
    if (a->dtype == KLAB_BF16) {
      if (a->K % 32) return KLAB_ERR_UNSUPPORTED;
      {  // d_model = 512: the A-stationary form (A in registers, only B streams through LDS); declines everything else
        const int rc = lmhead_areg_try(p, s);
        if (rc != KLAB_ERR_UNSUPPORTED) return rc;
      }
      size_t lds = KLAB_GLDS_STAGES * (size_t)(128 + 128) * 64;
      const size_t epi = (size_t)epilogue_lds_bytes<128, 128>(p.c_f32);
      return launch_kernel(klab_lmhead_gemm<bf16_t>, p, 128, 128, epi > lds ? epi : lds, s);
    }
    size_t lds = 2 * (size_t)(128 + 128) * ROWB;
    const size_t epi = (size_t)epilogue_lds_bytes<128, 128>(true);
    return launch_kernel(klab_lmhead_gemm<float>, p, 128, 128, epi > lds ? epi : lds, s);
  }
  // split-K with float atomics only for a plain accumulating f32 product (the wgrad form)
  const bool atomic_ok = a->atomic_ok && p.c_f32 && a->accumulate && !a->bias && !a->act && !a->aux && !a->residual && a->drop_p == 0.f;
  // name_tag 2: take the 256 x 256 eight-wave kernel whenever the shape is legal for it; 3: never (A/B, tests)
  const int p8_force = a->name_tag == 2 ? 1 : (a->name_tag == 3 ? -1 : 0);
  if (a->dtype == KLAB_BF16) return dispatch_tile<bf16_t>(p, atomic_ok, s, p8_force);
  return dispatch_tile<float>(p, atomic_ok, s);
}

extern "C" int klab_quant_fp8_rows(const void* x, long ldx, int M, int K, void* x8, long ld8, float* row_scale, void* stream) {
  using namespace klab;
  if (!x || !x8 || !row_scale) return KLAB_ERR_BADARG;
  if (M <= 0) return KLAB_OK;
  if (K <= 0 || K > 4096 || (K & 7) || (ldx & 7) || (ld8 & 7) || ((uintptr_t)x & 15) || ((uintptr_t)x8 & 7)) return KLAB_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(quant_fp8_rows_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, ldx, M, K,
                     (uint8_t*)x8, ld8, row_scale, 1L);
  KLAB_LAUNCH_CHECK();
  return KLAB_OK;
}

extern "C" int klab_quant_fp8_arena(const void* desc_dev, int ndesc, long total_rows, const void* arena_bf16, void* arena_fp8, float* scales,
                                    void* stream) {
  using namespace klab;
  if (!desc_dev || !arena_bf16 || !arena_fp8 || !scales || ndesc <= 0) return KLAB_ERR_BADARG;
  if (total_rows <= 0) return KLAB_OK;
  const long wgs = (total_rows + 3) / 4;
  hipLaunchKernelGGL(quant_fp8_arena_kernel, dim3((unsigned)(wgs < 4096 ? wgs : 4096)), dim3(256), 0, (hipStream_t)stream,
                     (const QuantDesc*)desc_dev, ndesc, total_rows, (const bf16_t*)arena_bf16, (uint8_t*)arena_fp8, scales);
  KLAB_LAUNCH_CHECK();
  return KLAB_OK;
}

extern "C" int klab_gemm_fp8(const klab_gemm_args* a, const float* a_row_scale, const float* b_row_scale, long b_scale_stride, void* stream) {
  using namespace klab;
  if (!a || !a->A || !a->B || !a->C || !a_row_scale || !b_row_scale) return KLAB_ERR_BADARG;
  if (a->M <= 0 || a->N <= 0 || a->K <= 0) return KLAB_OK;
  // A, B: fp8 bytes, K-major; everything else (C, aux, residual) as klab_gemm with dtype = KLAB_BF16
  if (a->dtype != KLAB_BF16 || !a->a_kmajor || !a->b_kmajor || a->accumulate) return KLAB_ERR_UNSUPPORTED;
  if ((a->K & 15) || (a->lda & 15) || (a->ldb & 15) || ((uintptr_t)a->A & 15) || ((uintptr_t)a->B & 15) || ((uintptr_t)a->C & 15))
    return KLAB_ERR_UNSUPPORTED;
  if (a->c_dtype != KLAB_F32 && a->c_dtype != KLAB_BF16) return KLAB_ERR_BADARG;
  GemmP p;
  fill_gemmp(a, p);
  Fp8Scales sc{a_row_scale, b_row_scale, b_scale_stride};
  hipStream_t s = (hipStream_t)stream;
  {  // the block-scaled instruction (2x the bf16 MFMA rate), opt-in (measured slower on this path's shapes: see mmf8.hip)
    const int rc = mmf8_try(p, a_row_scale, b_row_scale, b_scale_stride, a->name_tag == 2 ? 1 : (a->name_tag == 3 ? -1 : 0), s);
    if (rc != KLAB_ERR_UNSUPPORTED) return rc;
  }
  auto tiles = [&](int bm, int bn) { return (long)((p.M + bm - 1) / bm) * ((p.N + bn - 1) / bn); };
  // LDS-DMA ring form (whole 64-byte k-tiles, rows the DMA can address): the production path; the register-staged kernels below
  // take what is left (K % 64 != 0, tiny operands)
  if ((p.K % 64) == 0 && p.K >= 64 && p.M >= 16 && p.N >= 16) {
    p.splits = 1;
    const int nt = p.K / 64;
#define FP8_GLDS(BM_, BN_)                                                                                              \
    {                                                                                                                   \
      size_t lds = (size_t)(nt < KLAB_GLDS_STAGES ? nt : KLAB_GLDS_STAGES) * (BM_ + BN_) * 64;                          \
      const size_t epi = (size_t)epilogue_lds_bytes<BM_, BN_>(p.c_f32);                                                 \
      if (epi > lds) lds = epi;                                                                                         \
      int rc = ensure_dyn_lds(reinterpret_cast<const void*>(gemm_glds_fp8_kernel<BM_, BN_>), lds);                      \
      if (rc) return rc;                                                                                                \
      hipLaunchKernelGGL((gemm_glds_fp8_kernel<BM_, BN_>), dim3((unsigned)tiles(BM_, BN_)), dim3(256), lds, s, p, sc);   \
      KLAB_LAUNCH_CHECK();                                                                                              \
      return KLAB_OK;                                                                                                   \
    }
    if (tiles(128, 128) >= 240) FP8_GLDS(128, 128)
    if (tiles(128, 64) >= 240) FP8_GLDS(128, 64)
    FP8_GLDS(64, 64)
#undef FP8_GLDS
  }
  if (tiles(128, 128) >= 240) {
    size_t lds = 2 * (size_t)(128 + 128) * ROWB;
    const size_t epi = (size_t)epilogue_lds_bytes<128, 128>(p.c_f32);
    if (epi > lds) lds = epi;
    int rc = ensure_dyn_lds(reinterpret_cast<const void*>(gemm_fp8_kernel<128, 128>), lds);
    if (rc) return rc;
    hipLaunchKernelGGL((gemm_fp8_kernel<128, 128>), dim3((unsigned)tiles(128, 128)), dim3(256), lds, s, p, sc);
  } else {
    size_t lds = 2 * (size_t)(64 + 64) * ROWB;
    const size_t epi = (size_t)epilogue_lds_bytes<64, 64>(p.c_f32);
    if (epi > lds) lds = epi;
    int rc = ensure_dyn_lds(reinterpret_cast<const void*>(gemm_fp8_kernel<64, 64>), lds);
    if (rc) return rc;
    hipLaunchKernelGGL((gemm_fp8_kernel<64, 64>), dim3((unsigned)tiles(64, 64)), dim3(256), lds, s, p, sc);
  }
  KLAB_LAUNCH_CHECK();
  return KLAB_OK;
}
