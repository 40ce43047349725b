// T5 attention core (HF/t5:144-173 eager_attention_forward as called from HF/t5:281-369):
//   S = Q K^T * 1.0 + position_bias (+ causal mask in the decoder, HF/t5:697-711)
//   P = softmax(S);  Pd = dropout(P);  ctx = Pd V
// The q/k/v/o projections are klab_gemm calls; this file is the part between them, forward and
// backward, reading Q/K/V in place from the fused projection buffers (head h at column h*dk) and
// writing ctx / dQ / dK / dV in the same layouts, so no transpose or head split/merge is ever
// materialised.  K and V of one (batch, head) are staged in LDS once per workgroup; softmax
// statistics are fp32 with wave-shuffle reductions; backward recomputes P from the saved
// log-sum-exp (no [B,h,Lq,Lk] tensor is stored) and regenerates the dropout mask from the counter
// RNG.  The relative-position-bias gradient is accumulated with f32 atomics into [h,Lq,Lk].
// Round-1 form: dot products on the vector ALU in fp32 (sequence lengths here are 58-160; the
// contraction is 1.4 % of the step's FLOPs); an MFMA form is the planned replacement.
#include <math.h>

#include "common.h"
#include "klab_mm.h"

namespace klab {

struct AttnP {
  const void* q; long ldq;
  const void* k; long ldk;
  const void* v; long ldv;
  const float* bias;  // [H,Lq,Lk] or null
  int causal;
  void* ctx; long ldo;
  float* lse;         // [B,H,Lq]
  int B, H, Lq, Lk, dk;
  float p; const uint32_t* seed; uint32_t tag;
  // backward only
  const void* dctx; long lddo;
  void* dq; long lddq;
  void* dkk; long lddk;
  void* dv; long lddv;
  float* dbias;
};

constexpr int TQ = 16;

template <typename T> __device__ __forceinline__ void load_vec_f32(const T* p, float* o);
template <> __device__ __forceinline__ void load_vec_f32<float>(const float* p, float* o) {
  f32x4 v = *reinterpret_cast<const f32x4*>(p);
  o[0] = v[0]; o[1] = v[1]; o[2] = v[2]; o[3] = v[3];
}
template <> __device__ __forceinline__ void load_vec_f32<bf16_t>(const bf16_t* p, float* o) {
  bf16x8 v = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
  for (int i = 0; i < 8; ++i) o[i] = (float)v[i];
}

template <typename T>
__device__ __forceinline__ void stage_kv(const T* __restrict__ g, long ld, int b, int h, int Lk, int dk, T* lds, int stride) {
  constexpr int VEC = Vec16<T>::N;
  using V = typename Vec16<T>::type;
  const int cpr = dk / VEC;
  for (int ch = threadIdx.x; ch < Lk * cpr; ch += blockDim.x) {
    const int j = ch / cpr, c = (ch % cpr) * VEC;
    *reinterpret_cast<V*>(lds + j * stride + c) = *reinterpret_cast<const V*>(g + ((long)b * Lk + j) * ld + (long)h * dk + c);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void t5_attn_fwd_kernel(AttnP p) {
  constexpr int VEC = Vec16<T>::N;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int Lk = p.Lk, dk = p.dk, Lq = p.Lq;
  const int kst = dk + VEC;  // padded LDS row (elements)
  T* Ks = reinterpret_cast<T*>(smem);
  T* Vs = Ks + (size_t)Lk * kst;
  float* Qs = reinterpret_cast<float*>(Vs + (size_t)Lk * kst);
  float* Ps = Qs + TQ * dk;
  const int pst = Lk + 1;
  const int bh = blockIdx.y, b = bh / p.H, h = bh % p.H;
  const int q0 = blockIdx.x * TQ;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  stage_kv<T>(reinterpret_cast<const T*>(p.k), p.ldk, b, h, Lk, dk, Ks, kst);
  stage_kv<T>(reinterpret_cast<const T*>(p.v), p.ldv, b, h, Lk, dk, Vs, kst);
  const T* qg = reinterpret_cast<const T*>(p.q);
  for (int idx = tid; idx < TQ * dk; idx += 256) {
    const int i = idx / dk, c = idx % dk, qi = q0 + i;
    Qs[idx] = qi < Lq ? to_f32(qg[((long)b * Lq + qi) * p.ldq + (long)h * dk + c]) : 0.f;
  }
  __syncthreads();

  for (int idx = tid; idx < TQ * Lk; idx += 256) {
    const int i = idx / Lk, j = idx % Lk, qi = q0 + i;
    float s = -INFINITY;
    if (qi < Lq && !(p.causal && j > qi)) {
      s = 0.f;
      const T* kr = Ks + j * kst;
      const float* qr = Qs + i * dk;
      for (int c = 0; c < dk; c += VEC) {
        float kv[VEC];
        load_vec_f32<T>(kr + c, kv);
#pragma unroll
        for (int u = 0; u < VEC; ++u) s += qr[c + u] * kv[u];
      }
      if (p.bias) s += p.bias[((long)h * Lq + qi) * Lk + j];
    }
    Ps[i * pst + j] = s;
  }
  __syncthreads();

  const DropCtx dc = drop_slab(make_drop(p.seed, p.tag, p.p), (uint32_t)(b * p.H + h));
  for (int i = wave; i < TQ; i += 4) {
    const int qi = q0 + i;
    if (qi >= Lq) continue;
    float m = -INFINITY;
    for (int j = lane; j < Lk; j += 64) m = fmaxf(m, Ps[i * pst + j]);
    m = wave_max(m);
    float sum = 0.f;
    for (int j = lane; j < Lk; j += 64) sum += __expf(Ps[i * pst + j] - m);
    sum = wave_sum(sum);
    const float inv = 1.f / sum;
    if (lane == 0 && p.lse) p.lse[((long)b * p.H + h) * Lq + qi] = m + __logf(sum);
    const uint32_t base = (uint32_t)qi * (uint32_t)Lk;
    for (int j = lane; j < Lk; j += 64) Ps[i * pst + j] = __expf(Ps[i * pst + j] - m) * inv * drop_mult32(dc, base + j);
  }
  __syncthreads();

  T* og = reinterpret_cast<T*>(p.ctx);
  for (int idx = tid; idx < TQ * dk; idx += 256) {
    const int i = idx / dk, c = idx % dk, qi = q0 + i;
    if (qi >= Lq) continue;
    float o = 0.f;
    const float* pr = Ps + i * pst;
    for (int j = 0; j < Lk; ++j) o += pr[j] * to_f32(Vs[j * kst + c]);
    og[((long)b * Lq + qi) * p.ldo + (long)h * dk + c] = from_f32<T>(o);
  }
}

// Backward.  One workgroup per (batch, head).  The keys are visited in chunks of `kc` rows (kc = Lk whenever K, V and their f32
// gradient accumulators fit the 160 KB of LDS together; T5-large's cross-attention in fp32 parity mode, Lk = 153 at dk = 64, does
// not): per chunk, K / V rows are staged, every query tile is swept (P from the saved log-sum-exp, so no row needs its other
// chunks), dK / dV of the chunk are complete and stored, and dQ -- a sum over ALL keys -- is written by the first chunk and
// read-modify-written by the later ones (the same thread owns the same element every time: no race, fixed summation order).
template <typename T>
__global__ __launch_bounds__(256) void t5_attn_bwd_kernel(AttnP p, int kc) {
  constexpr int VEC = Vec16<T>::N;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int Lk = p.Lk, dk = p.dk, Lq = p.Lq;
  const int kst = dk + VEC, pst = kc + 1;
  T* Ks = reinterpret_cast<T*>(smem);
  T* Vs = Ks + (size_t)kc * kst;
  float* dKs = reinterpret_cast<float*>(Vs + (size_t)kc * kst);
  float* dVs = dKs + (size_t)kc * dk;
  float* Qs = dVs + (size_t)kc * dk;
  float* dOs = Qs + TQ * dk;
  float* Ps = dOs + TQ * dk;
  float* dSs = Ps + TQ * pst;
  float* delta = dSs + TQ * pst;
  float* lses = delta + TQ;
  const int bh = blockIdx.x, b = bh / p.H, h = bh % p.H;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const DropCtx dc = drop_slab(make_drop(p.seed, p.tag, p.p), (uint32_t)(b * p.H + h));
  const T* qg = reinterpret_cast<const T*>(p.q);
  const T* dog = reinterpret_cast<const T*>(p.dctx);
  const T* og = reinterpret_cast<const T*>(p.ctx);
  T* dqg = reinterpret_cast<T*>(p.dq);
  T* dkg = reinterpret_cast<T*>(p.dkk);
  T* dvg = reinterpret_cast<T*>(p.dv);
  const int cpr = dk / VEC;
  using V16 = typename Vec16<T>::type;

  for (int kb = 0; kb < Lk; kb += kc) {
    const int Lc = Lk - kb < kc ? Lk - kb : kc;
    __syncthreads();  // the previous chunk's images are fully consumed
    for (int ch = tid; ch < Lc * cpr; ch += 256) {
      const int j = ch / cpr, c = (ch % cpr) * VEC;
      const long row = (long)b * Lk + kb + j;
      *reinterpret_cast<V16*>(Ks + j * kst + c) = *reinterpret_cast<const V16*>(reinterpret_cast<const T*>(p.k) + row * p.ldk + (long)h * dk + c);
      *reinterpret_cast<V16*>(Vs + j * kst + c) = *reinterpret_cast<const V16*>(reinterpret_cast<const T*>(p.v) + row * p.ldv + (long)h * dk + c);
    }
    for (int idx = tid; idx < Lc * dk; idx += 256) { dKs[idx] = 0.f; dVs[idx] = 0.f; }

    for (int q0 = 0; q0 < Lq; q0 += TQ) {
      __syncthreads();  // previous tile fully consumed (and the chunk's staging visible)
      for (int idx = tid; idx < TQ * dk; idx += 256) {
        const int i = idx / dk, c = idx % dk, qi = q0 + i;
        float qv = 0.f, dov = 0.f;
        if (qi < Lq) {
          qv = to_f32(qg[((long)b * Lq + qi) * p.ldq + (long)h * dk + c]);
          dov = to_f32(dog[((long)b * Lq + qi) * p.lddo + (long)h * dk + c]);
        }
        Qs[idx] = qv; dOs[idx] = dov;
      }
      for (int i = wave; i < TQ; i += 4) {
        const int qi = q0 + i;
        float acc = 0.f;
        if (qi < Lq) {
          for (int c = lane; c < dk; c += 64)
            acc += to_f32(dog[((long)b * Lq + qi) * p.lddo + (long)h * dk + c]) * to_f32(og[((long)b * Lq + qi) * p.ldo + (long)h * dk + c]);
        }
        acc = wave_sum(acc);
        if (lane == 0) {
          delta[i] = acc;
          lses[i] = qi < Lq ? p.lse[((long)b * p.H + h) * Lq + qi] : 0.f;
        }
      }
      __syncthreads();

      for (int idx = tid; idx < TQ * Lc; idx += 256) {
        const int i = idx / Lc, j = idx % Lc, qi = q0 + i, kj = kb + j;
        float pd = 0.f, ds = 0.f;
        if (qi < Lq && !(p.causal && kj > qi)) {
          float s = 0.f, dpd = 0.f;
          const T* kr = Ks + j * kst;
          const T* vr = Vs + j * kst;
          const float* qr = Qs + i * dk;
          const float* dor = dOs + i * dk;
          for (int c = 0; c < dk; c += VEC) {
            float kv[VEC], vv[VEC];
            load_vec_f32<T>(kr + c, kv);
            load_vec_f32<T>(vr + c, vv);
#pragma unroll
            for (int u = 0; u < VEC; ++u) { s += qr[c + u] * kv[u]; dpd += dor[c + u] * vv[u]; }
          }
          if (p.bias) s += p.bias[((long)h * Lq + qi) * Lk + kj];
          const float pr = __expf(s - lses[i]);
          const float mlt = drop_mult32(dc, (uint32_t)qi * (uint32_t)Lk + kj);
          pd = pr * mlt;
          ds = pr * (dpd * mlt - delta[i]);
          if (p.dbias) atomicAdd(p.dbias + ((long)h * Lq + qi) * Lk + kj, ds);
        }
        Ps[i * pst + j] = pd;
        dSs[i * pst + j] = ds;
      }
      __syncthreads();

      for (int idx = tid; idx < Lc * dk; idx += 256) {
        const int j = idx / dk, c = idx % dk;
        float av = 0.f, ak = 0.f;
#pragma unroll 4
        for (int i = 0; i < TQ; ++i) {
          av += Ps[i * pst + j] * dOs[i * dk + c];
          ak += dSs[i * pst + j] * Qs[i * dk + c];
        }
        dVs[idx] += av;
        dKs[idx] += ak;
      }
      for (int idx = tid; idx < TQ * dk; idx += 256) {
        const int i = idx / dk, c = idx % dk, qi = q0 + i;
        if (qi >= Lq) continue;
        float a = 0.f;
        const float* dsr = dSs + i * pst;
        for (int j = 0; j < Lc; ++j) a += dsr[j] * to_f32(Ks[j * kst + c]);
        T* dst = dqg + ((long)b * Lq + qi) * p.lddq + (long)h * dk + c;
        if (kb > 0) a += to_f32(*dst);  // (this thread wrote the element for the earlier chunks)
        *dst = from_f32<T>(a);
      }
    }
    __syncthreads();
    for (int idx = tid; idx < Lc * dk; idx += 256) {
      const int j = idx / dk, c = idx % dk;
      dkg[((long)b * Lk + kb + j) * p.lddk + (long)h * dk + c] = from_f32<T>(dKs[idx]);
      dvg[((long)b * Lk + kb + j) * p.lddv + (long)h * dk + c] = from_f32<T>(dVs[idx]);
    }
  }
}

template <typename K>
static int set_lds(K kern, size_t bytes) { return ensure_dyn_lds(reinterpret_cast<const void*>(kern), bytes); }

}  // namespace klab

namespace klab {
int t5_attn_fwd_mfma_dispatch(const klab_attn_args* a, hipStream_t s);  // attn_t5_mfma.hip
int t5_attn_bwd_mfma_dispatch(const klab_attn_args* a, hipStream_t s);
int dbias_reduce_dispatch(const void* ds_ws, float* dbias, int nbatch, int H, int Lq, int Lk, hipStream_t s);
int t5_attn_fused_fwd_dispatch(const klab_attn_fused_args* fa, hipStream_t s);
}
using namespace klab;

static int check_attn(const klab_attn_args* a) {
  if (!a || !a->q || !a->k || !a->v || !a->ctx) return KLAB_ERR_BADARG;
  const int vec = a->dtype == KLAB_BF16 ? 8 : 4;
  if (a->dk % vec || a->ldq % vec || a->ldk % vec || a->ldv % vec) return KLAB_ERR_UNSUPPORTED;
  if (a->dtype != KLAB_F32 && a->dtype != KLAB_BF16) return KLAB_ERR_BADARG;
  return KLAB_OK;
}

static AttnP to_p(const klab_attn_args* a) {
  AttnP p;
  p.q = a->q; p.ldq = a->ldq; p.k = a->k; p.ldk = a->ldk; p.v = a->v; p.ldv = a->ldv;
  p.bias = a->bias; p.causal = a->causal; p.ctx = a->ctx; p.ldo = a->ldo; p.lse = a->lse;
  p.B = a->B; p.H = a->H; p.Lq = a->Lq; p.Lk = a->Lk; p.dk = a->dk;
  p.p = a->drop_p; p.seed = a->seed_dev; p.tag = a->drop_tag;
  p.dctx = a->dctx; p.lddo = a->lddo; p.dq = a->dq; p.lddq = a->lddq; p.dkk = a->dk_out; p.lddk = a->lddk;
  p.dv = a->dv; p.lddv = a->lddv; p.dbias = a->dbias;
  return p;
}

extern "C" int klab_t5_attn_fwd(const klab_attn_args* a, void* stream) {
  int rc = check_attn(a);
  if (rc) return rc;
  if (a->B <= 0 || a->Lq <= 0 || a->Lk <= 0) return KLAB_OK;
  if (a->score_scale || a->bias_mod) return KLAB_ERR_UNSUPPORTED;  // backward-only extensions (Swin window attention)
  if (a->dtype == KLAB_BF16) {  // matrix-core path first; fall through to the generic kernel outside its envelope
    rc = t5_attn_fwd_mfma_dispatch(a, (hipStream_t)stream);
    if (rc != KLAB_ERR_UNSUPPORTED) return rc;
  }
  const size_t es = a->dtype == KLAB_BF16 ? 2 : 4;
  const int vec = a->dtype == KLAB_BF16 ? 8 : 4;
  const size_t lds = 2 * (size_t)a->Lk * (a->dk + vec) * es + (size_t)TQ * a->dk * 4 + (size_t)TQ * (a->Lk + 1) * 4;
  AttnP p = to_p(a);
  dim3 grid((a->Lq + TQ - 1) / TQ, a->B * a->H);
  hipStream_t s = (hipStream_t)stream;
  if (a->dtype == KLAB_BF16) {
    rc = set_lds(t5_attn_fwd_kernel<bf16_t>, lds); if (rc) return rc;
    hipLaunchKernelGGL(t5_attn_fwd_kernel<bf16_t>, grid, dim3(256), lds, s, p);
  } else {
    rc = set_lds(t5_attn_fwd_kernel<float>, lds); if (rc) return rc;
    hipLaunchKernelGGL(t5_attn_fwd_kernel<float>, grid, dim3(256), lds, s, p);
  }
  KLAB_LAUNCH_CHECK();
  return KLAB_OK;
}

extern "C" int klab_t5_attn_fused_fwd(const klab_attn_fused_args* fa, void* stream) {
  if (!fa || !fa->x || !fa->gamma || !fa->w || !fa->xn || !fa->rstd || !fa->proj || !fa->attn.ctx) return KLAB_ERR_BADARG;
  if (fa->cross && (!fa->attn.k || !fa->attn.v)) return KLAB_ERR_BADARG;
  if (fa->attn.B <= 0) return KLAB_OK;
  return t5_attn_fused_fwd_dispatch(fa, (hipStream_t)stream);
}

extern "C" int klab_t5_attn_bwd(const klab_attn_args* a, void* stream) {
  int rc = check_attn(a);
  if (rc) return rc;
  if (!a->dctx || !a->dq || !a->dk_out || !a->dv || !a->lse) return KLAB_ERR_BADARG;
  if (a->B <= 0 || a->Lq <= 0 || a->Lk <= 0) return KLAB_OK;
  if (a->dtype == KLAB_BF16) {
    rc = t5_attn_bwd_mfma_dispatch(a, (hipStream_t)stream);
    if (rc != KLAB_ERR_UNSUPPORTED) return rc;
  }
  if (a->ds_defer) return KLAB_ERR_UNSUPPORTED;  // only the MFMA kernel stores dS; the caller retries without ds_defer
  if (a->score_scale || a->bias_mod) return KLAB_ERR_UNSUPPORTED;  // matrix-core kernel only (Swin window attention backward)
  const size_t es = a->dtype == KLAB_BF16 ? 2 : 4;
  const int vec = a->dtype == KLAB_BF16 ? 8 : 4;
  auto lds_for = [&](int kc) {
    return 2 * (size_t)kc * (a->dk + vec) * es + 2 * (size_t)kc * a->dk * 4 + 2 * (size_t)TQ * a->dk * 4 + 2 * (size_t)TQ * (kc + 1) * 4 + 2 * TQ * 4;
  };
  int kc = a->Lk;  // keys per chunk: all of them when the images fit, else the largest multiple of 16 that does
  const size_t budget = 150 * 1024;
  if (lds_for(kc) > budget) {
    kc = 16;
    while (kc + 16 < a->Lk && lds_for(kc + 16) <= budget) kc += 16;
    if (lds_for(kc) > budget) return KLAB_ERR_UNSUPPORTED;
  }
  const size_t lds = lds_for(kc);
  AttnP p = to_p(a);
  dim3 grid(a->B * a->H);
  hipStream_t s = (hipStream_t)stream;
  if (a->dtype == KLAB_BF16) {
    rc = set_lds(t5_attn_bwd_kernel<bf16_t>, lds); if (rc) return rc;
    hipLaunchKernelGGL(t5_attn_bwd_kernel<bf16_t>, grid, dim3(256), lds, s, p, kc);
  } else {
    rc = set_lds(t5_attn_bwd_kernel<float>, lds); if (rc) return rc;
    hipLaunchKernelGGL(t5_attn_bwd_kernel<float>, grid, dim3(256), lds, s, p, kc);
  }
  KLAB_LAUNCH_CHECK();
  return KLAB_OK;
}

extern "C" int klab_dbias_reduce(const void* ds_ws, int dtype, float* dbias, int nbatch, int H, int Lq, int Lk, void* stream) {
  if (!ds_ws || !dbias || dtype != KLAB_BF16) return KLAB_ERR_BADARG;
  return dbias_reduce_dispatch(ds_ws, dbias, nbatch, H, Lq, Lk, (hipStream_t)stream);
}

// ---- one-position decode attention with a K/V cache (greedy generation, ref/models/model.py:27-28; HF/t5:308-332) -----------
// One wave per (batch element, head): the single query row of position t against keys 0..Lk-1 held in the cache.
//   q  : row of sample b at q + b*q_bstride;   K/V: rows j of sample b at k + (b*kv_bstride + j*ldk)   (element strides)
//   bias_row: [H, bias_ld] values for THIS query position (relative-position bias row t), NULL for cross-attention
// Lanes split the keys (online softmax per lane, merged by a wave reduction); head dim 16 / 32 / 64 / 128, T = f32 | bf16.
namespace klab {
// Beam rows (klab_t5_beam_decode_attn): key j of query row r sits at row s*kv_bstride + j*ldk with s = kv_slot[r*slot_ld + j]
// (SLOT) or s = r / kv_group; the greedy call is kv_group 1 without a table (the same addresses, the same arithmetic).
template <typename T, int DK, bool SLOT>
__global__ __launch_bounds__(64) void decode_attn_kernel(const T* __restrict__ q, long q_bstride, const T* __restrict__ k, const T* __restrict__ v,
                                                         long kv_bstride, long ldk, int kv_group, const int* __restrict__ kv_slot, long slot_ld,
                                                         const float* __restrict__ bias_row, long bias_ld, T* __restrict__ ctx, long ctx_bstride,
                                                         int H, int Lk) {
  const int b = blockIdx.x / H, h = blockIdx.x % H, lane = threadIdx.x;
  const T* qr = q + (long)b * q_bstride + h * DK;
  const int kb = b / kv_group;
  float qv[DK], o[DK];
#pragma unroll
  for (int c = 0; c < DK; ++c) { qv[c] = to_f32(qr[c]); o[c] = 0.f; }
  float m = -INFINITY, l = 0.f;
  for (int j = lane; j < Lk; j += 64) {
    const long srow = SLOT ? (long)kv_slot[(long)b * slot_ld + j] : (long)kb;
    const T* kr = k + srow * kv_bstride + (long)j * ldk + h * DK;
    const T* vr = v + srow * kv_bstride + (long)j * ldk + h * DK;
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < DK; ++c) s += qv[c] * to_f32(kr[c]);  // unscaled scores (HF/t5:196-197)
    if (bias_row) s += bias_row[(long)h * bias_ld + j];
    const float mn = fmaxf(m, s), corr = __expf(m - mn), pe = __expf(s - mn);
    l = l * corr + pe;
#pragma unroll
    for (int c = 0; c < DK; ++c) o[c] = o[c] * corr + pe * to_f32(vr[c]);
    m = mn;
  }
  float mw = m;
#pragma unroll
  for (int s2 = 32; s2 > 0; s2 >>= 1) mw = fmaxf(mw, __shfl_xor(mw, s2, 64));
  const float f = (m == -INFINITY) ? 0.f : __expf(m - mw);
  float lw = l * f;
#pragma unroll
  for (int s2 = 32; s2 > 0; s2 >>= 1) lw += __shfl_xor(lw, s2, 64);
  const float il = 1.f / lw;
  T* orow = ctx + (long)b * ctx_bstride + h * DK;
#pragma unroll
  for (int c = 0; c < DK; ++c) {
    float x = o[c] * f;
#pragma unroll
    for (int s2 = 32; s2 > 0; s2 >>= 1) x += __shfl_xor(x, s2, 64);
    if (lane == 0) orow[c] = from_f32<T>(x * il);
  }
}
template <typename T>
static int launch_decode_attn(const void* q, long q_bstride, const void* k, const void* v, long kv_bstride, long ldk, int kv_group,
                              const int* kv_slot, long slot_ld, const float* bias_row, long bias_ld, void* ctx, long ctx_bstride, int B,
                              int H, int Lk, int dk, hipStream_t s) {
#define DEC_LAUNCH(D)                                                                                                              \
  if (kv_slot)                                                                                                                     \
    hipLaunchKernelGGL((decode_attn_kernel<T, D, true>), dim3(B * H), dim3(64), 0, s, (const T*)q, q_bstride, (const T*)k, (const T*)v, \
                       kv_bstride, ldk, kv_group, kv_slot, slot_ld, bias_row, bias_ld, (T*)ctx, ctx_bstride, H, Lk);              \
  else                                                                                                                             \
    hipLaunchKernelGGL((decode_attn_kernel<T, D, false>), dim3(B * H), dim3(64), 0, s, (const T*)q, q_bstride, (const T*)k, (const T*)v, \
                       kv_bstride, ldk, kv_group, kv_slot, slot_ld, bias_row, bias_ld, (T*)ctx, ctx_bstride, H, Lk)
  switch (dk) {
    case 8: DEC_LAUNCH(8); break;
    case 16: DEC_LAUNCH(16); break;
    case 32: DEC_LAUNCH(32); break;
    case 64: DEC_LAUNCH(64); break;
    case 128: DEC_LAUNCH(128); break;
    default: return KLAB_ERR_UNSUPPORTED;
  }
#undef DEC_LAUNCH
  KLAB_LAUNCH_CHECK();
  return KLAB_OK;
}
}  // namespace klab

extern "C" int klab_t5_beam_decode_attn(int dtype, const void* q, long q_bstride, const void* k, const void* v, long kv_bstride, long ldk,
                                        int kv_group, const int* kv_slot, long slot_ld, const float* bias_row, long bias_ld, void* ctx,
                                        long ctx_bstride, int R, int H, int Lk, int dk, void* stream) {
  using namespace klab;
  if (!q || !k || !v || !ctx || R <= 0 || H <= 0 || Lk <= 0 || kv_group < 1 || (kv_slot && slot_ld < Lk)) return KLAB_ERR_BADARG;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == KLAB_BF16)
    return launch_decode_attn<bf16_t>(q, q_bstride, k, v, kv_bstride, ldk, kv_group, kv_slot, slot_ld, bias_row, bias_ld, ctx, ctx_bstride, R, H,
                                      Lk, dk, s);
  if (dtype == KLAB_F32)
    return launch_decode_attn<float>(q, q_bstride, k, v, kv_bstride, ldk, kv_group, kv_slot, slot_ld, bias_row, bias_ld, ctx, ctx_bstride, R, H,
                                     Lk, dk, s);
  return KLAB_ERR_BADARG;
}
