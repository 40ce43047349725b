"""Fixtures and fp64 references for tests/test_gemm_exact_gpu.py, tests/test_attn_exact_gpu.py and tests/test_attn_fused_exact_gpu.py (plain torch on the CPU;
tests/test_exact_fixtures_cpu.py proves what the GPU tests take for granted about them).

GEMM: operands are integers in [-3, 3].  Every partial sum of a dot product is then an integer of magnitude <= 9 K < 2^24, so
the f32 result is the same in any summation order, through split-K atomics and through C += onto an integer C0, and
torch.equal with the fp64 product is a fair demand.  The epilogues that keep this property (scaling by 0.5, integer bias /
residual / C0, ReLU, the zero mask, dropout at p = 0.5) are evaluated in fp64 by gemm_expected.

T5 attention: softmax cannot be exact in general, but it is when every probability is a power of two.  The position bias is
-1000 everywhere except 0 on n in {1, 2, 4} chosen keys per (head, query), and the scores of the chosen keys of a row are equal
(n = 1: any Q, K; n > 1: Q = 0 or K = 0).  exp(-1000 + anything these operands can produce) is 0 in f32, so P is exactly 1/n on
the chosen keys and 0 elsewhere, and every output of forward and backward is a short sum of small dyadic numbers: exactly
representable in bf16 (checked in fp64 by the CPU test), so whatever a bf16 kernel stores must equal the reference bit for bit.
A second one-hot fixture needs no bias at all (the streaming kernels' BIAS = 0 instantiations): keys are distinct +-2 sign
codes and a query is 8 x its key, which puts every other score at least 128 below the chosen one.

Attention dropout: attn_drop_mult states the mask of the probabilities on its own (element (seed, tag, slab = b H + h, q Lk + key));
at p = 0.5 the multiplier is 0 or 2 and the dyadic fixtures stay dyadic (AttnFixture's `drop`).

The fused attention sub-layer kernels (tests/test_attn_fused_exact_gpu.py) reuse AttnFixture at head dim 64 for the backward, which is
handed dy and a signed-permutation o weight with dy @ W == rows(dO) (signed_perm, dy_for), and FusedFwdFixture for the forward: rows
sign * 2^k and one +-1 per k-tile in every projection row make the norm, the projection and the attention exact stage by stage.

Random operands: bounds are per element, the reference expression re-evaluated on absolute values times the unit roundoff of
the format (gemm_bound, attn_fwd_bound, attn_bwd_bounds; the derivation is in DESIGN.md section 1)."""
import functools
import math

import torch

U24 = 2.0 ** -24  # unit roundoff of f32
U8 = 2.0 ** -8    # unit roundoff of bf16: 8 significand bits, so round-to-nearest errs by up to half an ulp = 2^-8 relative just above a
                  # power of two (64.25 -> 64.5) and 2^-9 just below the next one; a perturbation below 2^-9 never survives the store
NEG = -1000.0     # position bias of a key that is not chosen


def gen(seed):
    return torch.Generator().manual_seed(seed)


def ints(g, lo, hi, *shape):
    """integers drawn uniformly from lo .. hi (inclusive) as fp64"""
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def bf16_exact(x):
    """does every element of the fp64 tensor survive a round trip through bf16?"""
    return bool((x.to(torch.bfloat16).double() == x).all())


def to_bf16_via_f32(x):
    """fp64 -> f32 -> bf16, each round-to-nearest-even: what a kernel that accumulates in f32 and stores bf16 must produce when
    the f32 value is exact"""
    return x.float().to(torch.bfloat16)


# ---- GEMM ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gemm_ints(M, N, K, seed=0):
    """A [M, K], B [N, K] (integers in [-3, 3], fp64) and the fp64 product A B^T.  Cached: the layouts, dtypes and epilogues of a
    shape share one reference; callers must not write into what they get."""
    g = gen(1000 + seed)
    A, B = ints(g, -3, 3, M, K), ints(g, -3, 3, N, K)
    return A, B, A @ B.T


@functools.lru_cache(maxsize=None)
def gemm_randn(M, N, K, seed=0):
    """randn operands rounded to bf16 (so that f32 and bf16 kernels are fed the same values), the fp64 product and the product
    of the absolute values"""
    g = gen(2000 + seed)
    A = torch.randn(M, K, generator=g).to(torch.bfloat16).double()
    B = torch.randn(N, K, generator=g).to(torch.bfloat16).double()
    return A, B, A @ B.T, A.abs() @ B.abs().T


def gemm_extras(M, N, seed=0):
    """integer epilogue operands for an [M, N] product: bias [N], residual [M, N], C0 [M, N], aux [M, N] (a third of it zero)"""
    g = gen(3000 + seed)
    aux = ints(g, -2, 2, M, N)
    aux[ints(g, 0, 2, M, N) == 0] = 0.0
    return dict(bias=ints(g, -4, 4, N), residual=ints(g, -8, 8, M, N), c0=ints(g, -8, 8, M, N), aux=aux)


def gemm_expected(prod, alpha=1.0, bias=None, relu=False, aux=None, aux_scale=1.0, residual=None, c0=None, row_scale=None,
                  col_scale=None):
    """the epilogue of klab_gemm / klab_gemm_fp8 in fp64, in the kernel's order: scales, bias, activation, zero mask, residual, C +="""
    x = prod * alpha
    if row_scale is not None:
        x = x * row_scale[:, None] * col_scale[None, :]
    if bias is not None:
        x = x + bias[None, :]
    if relu:
        x = x.clamp_min(0.0)
    if aux is not None:
        x = torch.where(aux != 0, x * aux_scale, torch.zeros_like(x))
    if residual is not None:
        x = x + residual
    if c0 is not None:
        x = x + c0
    return x


def gemm_bound(absprod, K, ref=None, bf16_out=False):
    """K f32 additions of exact products, doubled for faithful (not round-to-nearest) adds in the matrix unit:
    2 (K + 2) 2^-24 sum_k |a| |b|, plus one output rounding 2^-8 |ref| when C is bf16"""
    b = 2.0 * (K + 2) * U24 * absprod
    if bf16_out:
        b = b + U8 * ref.abs()
    return b


def fp8_gemm_bound(A, B, scale, absprod, K):
    """klab_gemm_fp8 on general e4m3 values.  The fp8 matrix instructions do not add their products in f32: within one instruction
    the products of a group of neighbouring k are aligned to the largest of the group and everything below 2^-13 of its leading bit
    is cut off (256 x 1 + 2^-3 x 2^-3 gives 256; 256 + 2^-5 is exact; the same through gemm_fp8_kernel, gemm_glds_fp8_kernel and
    mmf8_kernel -- test_fp8_products_within_13_bits_of_the_largest_are_kept pins the side the bound relies on).  Integer operands
    never notice, randn operands do.  Per product the cut is below 2^-13 max_k |a_mk| max_k |b_nk| whatever the grouping, hence
    K 2^-13 amax[m] bmax[n] on top of the f32 bound with two more multiplications (the row scales); all of it times the scales."""
    cut = K * 2.0 ** -13 * A.abs().amax(1)[:, None] * B.abs().amax(1)[None, :]
    return gemm_bound(absprod, K + 2) * scale + cut * scale


# ---- T5 attention: dyadic fixtures ---------------------------------------------------------------------------------------------
def chosen_keys(H, Lq, Lk, n, causal):
    """keys[h][q]: the chosen keys of a row (distinct, inside the causal prefix where causal applies).  A causal row with fewer than
    n visible keys takes the largest power of two that fits.  The keys of a row are spread evenly over what the row can see, the
    first key of the spread walks with q and h, row 0 takes key 0 and the last row the last key: the first and the last key and
    keys of different 32- and 64-key blocks all get picked."""
    keys = []
    for h in range(H):
        rows = []
        for q in range(Lq):
            avail = min(q + 1, Lk) if causal else Lk
            nq = n
            while nq > avail:
                nq //= 2
            start = (5 * q + 3 * h) % avail
            if q == 0:
                start = 0
            if q == Lq - 1:
                start = avail - 1
            if Lq == 1:  # a single row cannot take both ends: the heads share them out
                start = 0 if h == 0 else avail - 1 if h == H - 1 else (11 * h) % avail
            step = avail // nq
            rows.append(sorted((start + i * step) % avail for i in range(nq)))
        keys.append(rows)
    return keys


def sign_codes(g, L, dk):
    """L distinct rows of +-1 of length dk, any two of which differ in at least 2 places (row j carries j in its leading bits and
    the parity of those in the next one; the rest is random)"""
    nb = max(1, (L - 1).bit_length())
    assert nb + 1 <= dk
    c = torch.randint(0, 2, (L, dk), generator=g)
    j = torch.arange(L)
    for b in range(nb):
        c[:, b] = (j >> b) & 1
    c[:, nb] = c[:, :nb].sum(1) & 1
    return (2 * c - 1).double()


class AttnFixture:
    """One fixture at one shape.  Inputs q [B, H, Lq, dk], k, v [B, H, Lk, dk], do [B, H, Lq, dk] and bias [H, Lq, Lk] (or None),
    all fp64 and exactly representable in bf16; references P, dS [B, H, Lq, Lk], ctx, lse [B, H, Lq], dq, dk, dv and
    dbias [H, Lq, Lk], exact in fp64 by construction: P is written down (1 / n on the chosen keys), not computed through exp."""

    def __init__(self, kind, B, H, Lq, Lk, dk, causal=False, n=None, seed=0, drop=None):
        assert kind in ("onehot", "q0", "k0", "onehot_nobias")
        n = n or (1 if kind.startswith("onehot") else 2)
        assert (n == 1) == kind.startswith("onehot") and n in (1, 2, 4)
        self.kind, self.B, self.H, self.Lq, self.Lk, self.dk, self.causal, self.n = kind, B, H, Lq, Lk, dk, causal, n
        g = gen(4000 + seed)
        self.keys = chosen_keys(H, Lq, Lk, n, causal)
        mask = torch.zeros(H, Lq, Lk, dtype=torch.bool)
        for h in range(H):
            for q in range(Lq):
                mask[h, q, self.keys[h][q]] = True
        self.mask = mask
        cnt = mask.sum(-1, keepdim=True).double()
        self.P = (mask.double() / cnt)[None].expand(B, H, Lq, Lk).contiguous()
        self.q = ints(g, -2, 2, B, H, Lq, dk)
        self.k = ints(g, -2, 2, B, H, Lk, dk)
        self.v = ints(g, -1, 1, B, H, Lk, dk)
        self.do = ints(g, -1, 1, B, H, Lq, dk)
        self.bias = torch.where(mask, 0.0, NEG).double()
        if kind == "q0":
            self.q.zero_()
        elif kind == "k0":
            self.k.zero_()
        elif kind == "onehot_nobias":
            assert not causal
            self.bias = None
            self.k = 2.0 * torch.stack([torch.stack([sign_codes(g, Lk, dk) for _ in range(H)]) for _ in range(B)])
            idx = torch.tensor([[self.keys[h][q][0] for q in range(Lq)] for h in range(H)])
            self.q = 8.0 * torch.stack([torch.stack([self.k[b, h, idx[h]] for h in range(H)]) for b in range(B)])
        self.S = self.q @ self.k.transpose(-1, -2)  # [B, H, Lq, Lk] raw scores (integers)
        # the score every chosen key of a row shares (asserted by the CPU test), and with it the log-sum-exp
        chosen_score = torch.where(mask[None], self.S, -math.inf).amax(-1)
        self.lse = chosen_score + cnt[None, ..., 0].log()
        # drop = (seed, tag, p): the attention dropout mask M (0 or 1 / (1 - p)) on the probabilities, where the data path has it:
        # Pm = P M feeds the context and dV, dP is masked before delta is taken off (dS = P (dP M - delta), delta from the masked ctx)
        self.drop = drop
        self.M = torch.ones(B, H, Lq, Lk, dtype=torch.float64) if drop is None else attn_drop_mask(*drop, B, H, Lq, Lk)
        self.Pm = self.P * self.M
        self.ctx = self.Pm @ self.v
        dP = self.do @ self.v.transpose(-1, -2)
        delta = (self.do * self.ctx).sum(-1, keepdim=True)
        self.dS = self.P * (dP * self.M - delta)
        self.dq = self.dS @ self.k
        self.dk_ = self.dS.transpose(-1, -2) @ self.q
        self.dv = self.Pm.transpose(-1, -2) @ self.do
        self.dbias = self.dS.sum(0)

    def softmax_fp64(self):
        """P through the textbook route (scores + bias + causal mask -> softmax) in fp64, for the CPU test"""
        return attn_reference(self.q, self.k, self.v, self.bias, self.causal)[2]


@functools.lru_cache(maxsize=None)
def attn_fixture(kind, B, H, Lq, Lk, dk, causal=False, n=None, seed=0, drop=None):
    return AttnFixture(kind, B, H, Lq, Lk, dk, causal, n, seed, drop)


# ---- T5 attention: plain fp64 reference and per-element bounds -----------------------------------------------------------------
def attn_reference(q, k, v, bias, causal):
    """(ctx, lse, P) of HF T5 attention (unscaled scores + position bias, causal mask) in fp64; q [B, H, Lq, dk] etc."""
    S = q @ k.transpose(-1, -2)
    if bias is not None:
        S = S + bias[None]
    if causal:
        Lq, Lk = S.shape[-2:]
        S = S.masked_fill(torch.arange(Lk)[None, :] > torch.arange(Lq)[:, None], -math.inf)
    lse = torch.logsumexp(S, -1)
    P = (S - lse[..., None]).exp()
    return P @ v, lse, P


def attn_backward_reference(q, k, v, bias, causal, ctx, lse, do, M=None):
    """The backward as the function of what the kernel is handed: P = exp(S - lse) from the SAVED log-sum-exp and
    delta = rowsum(dO * ctx) from the SAVED context (both the forward kernel's outputs, as f32 / bf16 holds them), in fp64.
    Returns dq, dk, dv, dbias and the companions P, D (D >= |dS| element-wise: P (|dO| |V|^T + sum_d |dO ctx|)).
    M [B, H, Lq, Lk]: the dropout multipliers of the probabilities (attn_drop_mask): dV takes P M, dP is masked (dS = P (dP M - delta));
    the companions P and D then carry M where the data path does."""
    S = q @ k.transpose(-1, -2)
    if bias is not None:
        S = S + bias[None]
    P = (S - lse[..., None]).exp()
    if causal:
        Lq, Lk = S.shape[-2:]
        P = P.masked_fill(torch.arange(Lk)[None, :] > torch.arange(Lq)[:, None], 0.0)
    dP = do @ v.transpose(-1, -2)
    delta = (do * ctx).sum(-1, keepdim=True)
    if M is None:
        dS = P * (dP - delta)
        D = P * (do.abs() @ v.abs().transpose(-1, -2) + (do * ctx).abs().sum(-1, keepdim=True))
        return dict(dq=dS @ k, dk=dS.transpose(-1, -2) @ q, dv=P.transpose(-1, -2) @ do, dbias=dS.sum(0), P=P, D=D, dS=dS, P0=P)
    dS = P * (dP * M - delta)
    D = attn_ds_companion(P, M, v, ctx, do.abs())
    Pm = P * M
    return dict(dq=dS @ k, dk=dS.transpose(-1, -2) @ q, dv=Pm.transpose(-1, -2) @ do, dbias=dS.sum(0), P=Pm, D=D, dS=dS, P0=P)


def attn_ds_companion(P, M, v, ctx, e):
    """P (M (e |V|^T) + sum_d e |ctx|): what an element-wise magnitude (or error) e >= 0 of dO becomes in dS = P (dP M - delta)"""
    return P * (M * (e @ v.abs().transpose(-1, -2)) + (e * ctx.abs()).sum(-1, keepdim=True))


def attn_fwd_bound(P, v):
    """bf16 kernels: P is rounded to bf16 before P V (2^-8 per term) and the f32 sum is rounded to bf16 once (2^-8 of a value that
    is at most sum_k p |v|): 2^-7 sum_k p_k |v_kd|, with nothing added for the f32 terms (exp, the normaliser, the sum)."""
    return 2.0 * U8 * (P @ v.abs())


def attn_f32_factor(q, k, Lk, dk):
    """f32 kernels (and the f32 part of every bf16 kernel), as a RELATIVE error of one probability: the score is a sum of dk
    products ((dk + 2) 2^-24 |q|.|k| absolute, which exp turns into a relative error), exp / log / reciprocal at a few ulp, the
    normaliser a sum of Lk terms.  Doubled like gemm_bound.  Shape [B, H, Lq, Lk]."""
    return 2.0 * U24 * ((dk + 2) * (q.abs() @ k.abs().transpose(-1, -2)) + Lk + 16)


def attn_bwd_bounds(r, q, k, v, do, Lq, Lk, dk, B, stored_ds):
    """Per-element bounds for the bf16 MFMA / streaming backward kernels: the bf16 roundings on each output's data path, 2^-8 each,
    on the companion of the output, plus the f32 terms of attn_f32_bounds:
      dv    = bf16(sum_q bf16(P) dO):   P, store                 -> 2 roundings on P^T |dO|
      dq    = bf16(sum_k bf16(dS) K):   dS, store                -> 2 roundings on D |K|
      dk    = bf16(sum_q bf16(dS) Q):   dS, store                -> 2 roundings on D^T |Q|
      dbias = sum_b bf16(dS) (stored-dS slab, f32 reduce)        -> 1 rounding on sum_b D; none with float atomics
    dO, Q, K, V are inputs (already bf16), delta and dP are f32.  No further margin."""
    P, D = r["P"], r["D"]
    f = attn_f32_bounds(r, q, k, v, do, Lq, Lk, dk, B)
    return dict(dv=2.0 * U8 * (P.transpose(-1, -2) @ do.abs()) + f["dv"], dq=2.0 * U8 * (D @ k.abs()) + f["dq"],
                dk=2.0 * U8 * (D.transpose(-1, -2) @ q.abs()) + f["dk"], dbias=(U8 * D.sum(0) if stored_ds else 0.0) + f["dbias"])


def attn_f32_bounds(r, q, k, v, do, Lq, Lk, dk, B):
    """The f32 kernels: every quantity carries the relative error of P (attn_f32_factor, taken at its row / column maximum where a
    sum runs over it) plus one f32 addition per term of its own sums, doubled."""
    P, D = r["P"], r["D"]
    f = attn_f32_factor(q, k, Lk, dk)
    n = 2.0 * U24 * (2 * dk + Lq + Lk + B + 8)
    fP, fD = (f + n) * P, (f + n) * D
    return dict(ctx=fP @ v.abs(), dv=fP.transpose(-1, -2) @ do.abs(), dq=fD @ k.abs(), dk=fD.transpose(-1, -2) @ q.abs(), dbias=fD.sum(0))


@functools.lru_cache(maxsize=None)
def attn_randn(B, H, Lq, Lk, dk, causal, with_bias, seed=0):
    """randn q, k, v, dO rounded to bf16 (fp64 holds them), a position bias of a few units, and the forward reference"""
    g = gen(5000 + seed)
    r = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16).double()
    q, k, v, do = r(B, H, Lq, dk) * 0.5, r(B, H, Lk, dk) * 0.5, r(B, H, Lk, dk), r(B, H, Lq, dk)
    bias = (2.0 * torch.randn(H, Lq, Lk, generator=g)).float().double() if with_bias else None
    ctx, lse, P = attn_reference(q, k, v, bias, causal)
    return dict(q=q, k=k, v=v, do=do, bias=bias, ctx=ctx, lse=lse, P=P)


# ---- the shapes: the smallest the dispatcher sends to each kernel --------------------------------------------------------------
# Every M and N below is ragged (no multiple of 16) and a multiple of 8, so that each shape is legal in all four operand
# layouts (an m-major bf16 operand needs its contiguous dimension to be a multiple of 8).  Rules quoted from dispatch_tile
# (gemm.hip): tiles(bm, bn) = ceil(M / bm) ceil(N / bn), nt = ceil(K / BK) with BK = 64 (bf16) / 32 (f32), TILE_MIN = 224.
# bf16 with K % 32 == 0 runs the LDS-DMA ring kernel gemm_glds_kernel, any other K (and all of f32) the register-staged
# gemm_kernel (dispatch_layout): every four-wave tile is therefore visited with K = 64 / 96 / 320 and with K = 72 / 328.
T64 = (136, 88)       # tiles(128, 64) = 4 < 224, no atomics                        -> 64 x 64
T64_ODD = (77, 91)    # the same tile with odd M, N (k-major operands only): the scalar copy-out path
T128x64 = (1896, 968)   # tiles(128, 128) = 15 * 8 = 120 < 224 <= tiles(128, 64) = 15 * 16 = 240 -> 128 x 64
T128 = (1896, 1928)     # tiles(128, 128) = 15 * 16 = 240 >= 224                     -> 128 x 128
# 256 x 128 eight-wave kernel (gemm_glds_w8_kernel): bf16, A k-major, K >= 1024, K % 32 == 0, M >= 256, N >= 128,
# tiles(128, 128) = 17 * 16 = 272 > 256 and tiles(256, 128) = 9 * 16 = 144 <= 256
W8 = (2056, 1928, 1024)
# split-K with float atomics (f32 C, accumulate, atomic_ok, no epilogue extras):
#   nt >= 16, not (M >= 128 and N >= 64): 64 x 64 form;  M >= 128 and N >= 64: 128 x 64 form, splits = min(ceil(256 / tiles), nt / 8, 16)
#   nt >= 256, M >= 128, N >= 64: long-K form, 128 x 128 tiles when N >= 128 else 128 x 64, splits = min(ceil(1024 / tiles), nt / 64, 16)
SPLITK = {
    # name: (M, N, {dtype: K values})
    "sk64": (72, 88, {"bf16": (2080, 2088), "f32": (1000,)}),         # bf16 nt = 33 -> 4 splits (ring / register-staged); f32 nt = 32 -> 4
    "sk128x64": (136, 88, {"bf16": (2080, 2088), "f32": (1000,)}),    # tiles(128, 64) = 4 -> min(64, nt / 8) = 4 splits
    "sk_long128": (136, 136, {"bf16": (16384,), "f32": (8192,)}),     # nt = 256, tiles(128, 128) = 4 -> min(256, 4, 16) = 4 splits
    "sk_long128x64": (136, 88, {"bf16": (16384,), "f32": (8192,)}),   # N < 128: the 128 x 64 tile of the same rule
}
# 256 x 256 kernel (mm8p_try with name_tag = 2: K % 64 == 0, K >= 128, m-major operands a multiple of 8): 2 x 3 tiles, both edges
# ragged; K = 192 is three k-tiles (odd); split-K: tiles * 2 * splits <= 256 and nt / (2 splits) >= 8 -> K = 1088 (17 k-tiles): 2 splits
P8 = (264, 520)
# name_tag = 1 (both operands k-major): klab_lmhead_gemm<float> / <bf16> at any shape; the A-stationary lmhead_areg kernel takes
# bf16 -> bf16, K = 512, M >= 1024, N >= MIN_N = 8192 and N % 128 == 0, and declines everything else (N = 1928 below)
LMHEAD_SMALL = (136, 200)
LMHEAD_AREG = (1032, 8192, 512)
LMHEAD_DECLINED = (1032, 1928, 512)
# fp8 (klab_gemm_fp8, K % 16 == 0): K % 64 != 0 -> register-staged gemm_fp8_kernel (128 x 128 when tiles(128, 128) >= 240, else
# 64 x 64); K % 64 == 0 -> ring gemm_glds_fp8_kernel (128 x 128 / 128 x 64 at >= 240 tiles, else 64 x 64); name_tag = 2 and
# K % 128 == 0 -> block-scaled mmf8_kernel with the same three tiles
FP8 = {
    "staged64": (136, 88, 80, 0), "staged128": (1896, 1928, 80, 0),
    "ring64": (136, 88, 192, 0), "ring128x64": (1896, 1032, 192, 0), "ring128": (1896, 1928, 64, 0),
    "scaled64": (136, 88, 384, 2), "scaled128x64": (1896, 1032, 128, 2), "scaled128": (1896, 1928, 256, 2),
}
# the epilogue family runs on a 4 x 3 grid of 64 x 64 tiles: interior tiles (the vector fast path of copy_out_tile) and ragged ones
EPI = (200, 152)


def gemm_shapes():
    """every (M, N, K) the exact GEMM tests use, for the CPU test"""
    s = set()
    for M, N in (T64, T128x64, T128):
        s |= {(M, N, K) for K in (64, 72, 96, 320, 328)}
    s |= {(*T64_ODD, 72), (*T64_ODD, 96), W8, LMHEAD_AREG, LMHEAD_DECLINED, (*LMHEAD_SMALL, 72), (*LMHEAD_SMALL, 96)}
    for M, N, ks in SPLITK.values():
        s |= {(M, N, K) for v in ks.values() for K in v}
    s |= {(*P8, 192), (*P8, 1088), (*EPI, 72), (*EPI, 96), (*EPI, 192)}
    s |= {(M, N, K) for M, N, K, _ in FP8.values()}
    return sorted(s)


# T5 attention.  (Lq, Lk, dk, causal); B = 3 (the float-atomics bias gradient wants more than two batch elements), H = 2.
# One-workgroup MFMA forward t5_attn_fwd_mfma<dk, MT>: bf16, dk in {16, 32, 64, 128}, MT = 4 / 8 / 16 for Lk padded to 32 of at
# most 64 / 128 / 256 -> Lk = 58 / 69 / 153; a workgroup owns 64 queries, so Lq = 70 and the causal 69 / 153 have several query tiles.
# One-workgroup MFMA backward t5_attn_bwd_mfma<dk>: the same shapes while its images fit 160 KiB of LDS (mfma_bwd_fits); the
# others fall through to the generic bf16 kernel of attn_t5.hip (dk = 128, causal) and are compared all the same.
ATTN_MFMA = [(33, 58, 16, False), (70, 58, 32, False), (33, 58, 64, False), (70, 58, 128, False),
             (70, 69, 16, False), (33, 69, 32, False), (70, 69, 64, False), (33, 69, 128, False),
             (33, 153, 16, False), (70, 153, 32, False), (70, 153, 64, False), (33, 153, 128, False),
             (58, 58, 64, True), (58, 58, 16, True), (69, 69, 64, True), (69, 69, 128, True), (153, 153, 64, True), (153, 153, 32, True)]
# Streaming kernels flash_fwd / flash_bwd_dq / flash_bwd_dkv: not causal, dk in {32, 64}; forward when Lk padded exceeds 256,
# backward when the one-workgroup images do not fit.  Four query blocks and five key blocks of 64, both ragged.
ATTN_FLASH = [(200, 300, 32, False), (200, 300, 64, False)]
# Generic kernels of attn_t5.hip: f32 always (Lq = 21, 37: no multiple of TQ = 16), bf16 at a head dim outside the MFMA set;
# (33, 153, 64) in f32 needs 1184 bytes of LDS per key + 8.4 KiB against a budget of 150 KiB: chunks of kc = 112 < Lk keys
ATTN_GENERIC = [("f32", 21, 37, 16, False), ("f32", 37, 37, 32, True), ("bf16", 33, 58, 24, False), ("f32", 33, 153, 64, False)]
ATTN_B, ATTN_H = 3, 2
# the one-workgroup MFMA kernels once more under dropout (p = 0.5, FUSED_DROP below): the mask of exact_ref.attn_drop_mult
ATTN_DROP = [(33, 58, 64, False), (58, 58, 64, True)]



def fixtures_for(dk):
    """(kind, n): q0 has four chosen keys per row up to head dim 32 and two above it -- with n = 4 and 64 or more terms in dO . V
    the 1/16ths of dS times K no longer fit the 8 significand bits of bf16 at every shape; k0 always has two, since dK sums dS over
    all the rows that chose a key (the CPU test is the judge of both)"""
    return (("onehot", 1), ("q0", 4 if dk <= 32 else 2), ("k0", 2))


def mfma_bwd_fits(Lq, Lk, dk):
    """launch_bwd's LDS size (attn_t5_mfma.hip) against ensure_dyn_lds' limit"""
    dkp = max(32, (dk + 31) // 32 * 32)
    pd = {128: 72, 64: 40, 32: 24}[dkp]
    groupb = (8 * pd + 32) * 4
    lqp, lkp = (Lq + 31) // 32 * 32, (Lk + 31) // 32 * 32
    return (2 * lqp + 2 * lkp) * (dkp * 2 + 16) + (2 * (lqp // 8) + lkp // 8) * groupb + 2 * lqp * 4 <= 160 * 1024


def attn_fixture_cases():
    """every (kind, n, Lq, Lk, dk, causal) of the exact attention tests"""
    out = []
    for Lq, Lk, dk, causal in ATTN_MFMA + ATTN_FLASH + [c[1:] for c in ATTN_GENERIC]:
        out += [(kind, n, Lq, Lk, dk, causal) for kind, n in fixtures_for(dk)]
    out += [("onehot_nobias", 1, Lq, Lk, dk, causal) for Lq, Lk, dk, causal in ATTN_FLASH]
    return out


# ---- attention dropout ---------------------------------------------------------------------------------------------------------
def attn_drop_mult(seed, tag, p, slab, off):
    """The multiplier of probability `off` = q * Lk + key of slab b * H + h, stated on its own (csrc/common.h): the key of
    make_drop(seed, tag), folded with the slab by drop_slab, then one hash round on the 32-bit offset (drop_mult32):
    mix32(off * 0x9E3779B1 + key) < trunc(p 2^32) ? 0 : 1 / (1 - p), f32.  slab and off are integer arrays that broadcast."""
    import numpy as np
    from tests.rowops_ref import mix32  # (rowops_ref imports this module at its top)
    m = np.uint64(0xFFFFFFFF)
    key = mix32(np.uint64((int(seed) * 0x9E3779B1 + int(tag) * 0x7FEB352D + 0x165667B1) & 0xFFFFFFFF))
    slab = np.asarray(slab).astype(np.uint64) & m
    key = mix32(key ^ ((slab * np.uint64(0x85EBCA77) + np.uint64(0x27D4EB2F)) & m))
    off = np.asarray(off).astype(np.uint64) & m
    h = mix32((off * np.uint64(0x9E3779B1) + key) & m)
    pf = np.float32(p)
    thresh = min(int(float(pf) * 4294967296.0), 0xFFFFFFFF)
    scale = np.float32(1.0) / (np.float32(1.0) - pf)
    return np.where(h < np.uint64(thresh), np.float32(0.0), scale).astype(np.float32)


def attn_drop_mask(seed, tag, p, B, H, Lq, Lk):
    """M [B, H, Lq, Lk] (fp64 holding the f32 multipliers) of one attention call"""
    import numpy as np
    slab = (np.arange(B)[:, None] * H + np.arange(H)[None, :])[:, :, None, None]
    off = (np.arange(Lq)[:, None] * Lk + np.arange(Lk)[None, :])[None, None]
    return torch.from_numpy(attn_drop_mult(seed, tag, p, slab, off)).double()


# ---- fused T5 attention sub-layer kernels (klab_t5_attn_fused_fwd, klab_t5_attn_bwd_fused) --------------------------------------
# d_model = 512, head dim 64, at most 64 queries / keys.  (cross, B, H, Lq, Lk, causal): the smallest shapes that reach every branch --
# 64 (full tiles), 58 (ragged last wave), 33 (NS / NQS = 2 by one row), 17 (one wave + one row, NS = NQS = 1), 5 (three waves
# without a query), 1; cross with Lq != Lk on either side of 32; B = 3 (the plain workgroup -> (sample, head) map) and B = 16 (the
# (B & 7) == 0 map, two groups of eight samples).
FUSED_D, FUSED_DK = 512, 64
FUSED_SELF = [(64, True), (58, False), (33, True), (17, False), (5, True), (1, False)]
FUSED_CROSS = [(64, 58), (40, 64), (9, 33), (33, 9), (1, 64), (64, 1)]
FUSED_SHAPES = ([(False, 3, 8, L, L, c) for L, c in FUSED_SELF] + [(True, 3, 8, Lq, Lk, False) for Lq, Lk in FUSED_CROSS]
                + [(False, 16, 8, 58, 58, False), (True, 16, 8, 64, 58, False)])
# the forward's envelope fixes d_model and the head dim only: Flan-T5-small has 6 heads (inner = 384)
FUSED_FWD_SHAPES = FUSED_SHAPES + [(False, 3, 6, 33, 33, True), (True, 3, 6, 40, 64, False)]
FUSED_RANDOM = [(cross, B, 8, Lq, Lk, c) for B in (3, 16) for cross, Lq, Lk, c in
                ((False, 64, 64, True), (False, 58, 58, False), (True, 64, 58, False), (True, 9, 33, False))]
FUSED_DROP = (31, 11, 0.5)         # (seed, tag, p) of the exact dropout cases: the multiplier is 0 or 2, dyadic stays dyadic
FUSED_RANDOM_DROP = (31, 11, 0.1)
FUSED_FWD_KINDS = (("onehot", 1), ("q0", 4), ("k0", 2))  # (the CPU test is the judge of n, as for fixtures_for)
FUSED_NEG = -65536.0  # bias of a key that is not chosen: |S| <= 64 * 16 * 16 = 2^14, so S + NEG is an integer f32 holds and
                      # NEG + max S - min S <= -2^15: exp of it is 0 in f32 (and in fp64)


def heads(x, L, H):
    """[B * L, H * dk] -> [B, H, L, dk]"""
    n, hd = x.shape
    return x.reshape(n // L, L, H, hd // H).permute(0, 2, 1, 3)


def unheads(x):
    """[B, H, L, dk] -> [B * L, H * dk]: head h at column h * dk"""
    b, h, L, dk = x.shape
    return x.permute(0, 2, 1, 3).reshape(b * L, h * dk)


@functools.lru_cache(maxsize=None)
def signed_perm(d=FUSED_D, tile=64, seed=0):
    """The o / co projection weight of the exact backward cases: W [d, d] (nn.Linear layout [d_model, inner]) with one +-1 per row
    and per column, W[n, pi[n]] = sign[n].  Of the 64 rows of every k-tile of the dgrad (rows 64 t .. + 63) eight go to each head's
    64-column slice, at random places of the tile and of the slice.  -> (W, pi, sign)"""
    g = gen(6000 + seed)
    nt = d // tile
    per = tile // nt
    slots = [torch.randperm(tile, generator=g) for _ in range(nt)]
    pi = torch.empty(d, dtype=torch.int64)
    for t in range(nt):
        r = torch.randperm(tile, generator=g) + t * tile
        for h in range(nt):
            pi[r[h * per:(h + 1) * per]] = h * tile + slots[h][t * per:(t + 1) * per]
    sign = 2.0 * torch.randint(0, 2, (d,), generator=g).double() - 1.0
    W = torch.zeros(d, d, dtype=torch.float64)
    W[torch.arange(d), pi] = sign
    return W, pi, sign


def dy_for(do):
    """dy [B * Lq, 512] with dy @ W == rows(dO) exactly for W = signed_perm(): dy = rows(dO) W^T (a signed shuffle of the columns)"""
    return unheads(do) @ signed_perm()[0].T


@functools.lru_cache(maxsize=None)
def fused_bwd_fixture(kind, n, cross, B, H, Lq, Lk, causal, drop=None):
    """AttnFixture at head dim 64 (cached: callers must not write into it)"""
    return AttnFixture(kind, B, H, Lq, Lk, FUSED_DK, causal, n, 0, drop)


class FusedFwdFixture:
    """klab_t5_attn_fused_fwd on operands that make every stage exact.
    x[r, c] = sign[r, c] s_r with s_r in {1, 2, 4}: mean(x^2) = s_r^2 and x * rstd is within a few 1e-7 of +-1; gamma in {1, 2}:
    bf16(gamma (x rstd)) = sign gamma for every rstd the rstd bound admits (the CPU test shows it).  Every projection row has one
    +-1 in each of the eight k-tiles of 64 columns, so q | k | v are integers of magnitude <= 16, exact in f32 in any order and in
    bf16.  The attention is AttnFixture's: bias 0 on the chosen keys and FUSED_NEG elsewhere; n = 1 for any q, k ('onehot'), n > 1
    with the q block ('q0') or the k block ('k0': cross attention zeroes the given K) of the weight zero.  In the cross form K and
    V are inputs, drawn as AttnFixture draws them.  References (fp64): xn [B Lq, 512], rstd [B Lq], proj [B Lq, 3 inner | inner],
    P, M, Pm [B, H, Lq, Lk], ctx [B, H, Lq, 64], lse [B, H, Lq]."""

    def __init__(self, kind, n, cross, B, H, Lq, Lk, causal, drop=None, eps=1e-6):
        assert kind in ("onehot", "q0", "k0") and (n == 1) == (kind == "onehot") and (cross or Lq == Lk)
        d, dk = FUSED_D, FUSED_DK
        inner = H * dk
        self.kind, self.n, self.cross, self.B, self.H, self.Lq, self.Lk, self.causal, self.inner = kind, n, cross, B, H, Lq, Lk, causal, inner
        g = gen(8000 + 7 * Lq + Lk + 1000 * H)
        nrows = B * Lq
        sign = 2.0 * torch.randint(0, 2, (nrows, d), generator=g).double() - 1.0
        self.s = 2.0 ** torch.randint(0, 3, (nrows,), generator=g).double()
        self.x = sign * self.s[:, None]
        self.gamma = 1.0 + torch.randint(0, 2, (d,), generator=g).double()
        self.eps = eps
        self.rstd = (self.x.pow(2).mean(-1) + eps).rsqrt()
        self.xn = sign * self.gamma[None, :]
        nproj = inner if cross else 3 * inner
        W = torch.zeros(nproj, d, dtype=torch.float64)
        for t in range(d // 64):
            col = t * 64 + torch.randint(0, 64, (nproj,), generator=g)
            W[torch.arange(nproj), col] = 2.0 * torch.randint(0, 2, (nproj,), generator=g).double() - 1.0
        if kind == "q0":
            W[:inner] = 0.0
        elif kind == "k0" and not cross:
            W[inner:2 * inner] = 0.0
        self.w = W
        self.proj = self.xn @ W.T
        self.q = heads(self.proj[:, :inner], Lq, H)
        if cross:
            self.k = ints(g, -2, 2, B, H, Lk, dk)
            self.v = ints(g, -1, 1, B, H, Lk, dk)
            if kind == "k0":
                self.k.zero_()
        else:
            self.k = heads(self.proj[:, inner:2 * inner], Lk, H)
            self.v = heads(self.proj[:, 2 * inner:], Lk, H)
        self.keys = chosen_keys(H, Lq, Lk, n, causal)
        mask = torch.zeros(H, Lq, Lk, dtype=torch.bool)
        for h in range(H):
            for q in range(Lq):
                mask[h, q, self.keys[h][q]] = True
        self.mask = mask
        cnt = mask.sum(-1, keepdim=True).double()
        self.P = (mask.double() / cnt)[None].expand(B, H, Lq, Lk).contiguous()
        self.bias = torch.where(mask, 0.0, FUSED_NEG).double()
        self.S = self.q @ self.k.transpose(-1, -2)
        self.lse = torch.where(mask[None], self.S, -math.inf).amax(-1) + cnt[None, ..., 0].log()
        self.M = torch.ones(B, H, Lq, Lk, dtype=torch.float64) if drop is None else attn_drop_mask(*drop, B, H, Lq, Lk)
        self.Pm = self.P * self.M
        self.ctx = self.Pm @ self.v

    def softmax_fp64(self):
        return attn_reference(self.q, self.k, self.v, self.bias, self.causal)[2]


@functools.lru_cache(maxsize=None)
def fused_fwd_fixture(kind, n, cross, B, H, Lq, Lk, causal, drop=None):
    return FusedFwdFixture(kind, n, cross, B, H, Lq, Lk, causal, drop)


def rstd_bound(ref, d=FUSED_D):
    """(adds(d) + 8) 2^-24 |ref|: the longest chain of f32 additions of a 64-lane row sum (rowops_ref.adds) plus the division, eps,
    the reciprocal square root and slack for their ulps -- the bound tests/test_norm_exact_gpu.py holds klab_rmsnorm_fwd to"""
    from tests.rowops_ref import adds
    return (adds(d) + 8) * U24 * ref.abs()


@functools.lru_cache(maxsize=None)
def fused_randn(cross, B, H, Lq, Lk):
    """random operands of both fused kernels (bf16 / f32 values held in fp64): x, gamma, the projection weight, the given K | V of
    the cross form, the position bias; q | k | v, dy and the o weight of the backward"""
    g = gen(9000 + 100 * Lq + Lk + B)
    d, inner = FUSED_D, H * FUSED_DK
    r16 = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16).double()
    r32 = lambda *s: torch.randn(*s, generator=g).float().double()
    return dict(x=2.0 * r32(B * Lq, d), gamma=(1.0 + 0.1 * torch.randn(d, generator=g)).float().double(),
                w=(torch.randn((1 if cross else 3) * inner, d, generator=g) * d ** -0.5).to(torch.bfloat16).double(),
                k=0.5 * r16(B, H, Lk, FUSED_DK), v=r16(B, H, Lk, FUSED_DK), bias=(2.0 * torch.randn(H, Lq, Lk, generator=g)).float().double(),
                q=0.5 * r16(B, H, Lq, FUSED_DK), dy=r16(B * Lq, d), wo=(torch.randn(d, inner, generator=g) * d ** -0.5).to(torch.bfloat16).double())


def attn_bwd_fused_bounds(r, M, q, k, v, ctx, do, absdo, Lq, Lk, dk, B, stored_ds):
    """klab_t5_attn_bwd_fused: attn_bwd_bounds (with P M where the data path has it: r from attn_backward_reference(..., M)) plus
    the error of the kernel's own dO = bf16(dy W_h) against the fp64 product the reference is given:
        e = 2^-8 |dO| + gemm_bound(|dy| |W_h|, 512)        (one rounding to bf16, 512 f32 additions of exact products)
    pushed once through every expression that contains dO: (P M)^T e for dV; for dS = P (dP M - delta) both dP = dO V^T and
    delta = rowsum(dO ctx) carry it, E = P (M (e |V|^T) + sum_d e |ctx|), hence E |K| for dQ, E^T |Q| for dK, sum_b E for dbias."""
    b = attn_bwd_bounds(r, q, k, v, do, Lq, Lk, dk, B, stored_ds)
    e = U8 * do.abs() + gemm_bound(absdo, FUSED_D)
    E = attn_ds_companion(r["P0"], M, v, ctx, e)
    return dict(dv=b["dv"] + r["P"].transpose(-1, -2) @ e, dq=b["dq"] + E @ k.abs(), dk=b["dk"] + E.transpose(-1, -2) @ q.abs(),
                dbias=b["dbias"] + E.sum(0))
