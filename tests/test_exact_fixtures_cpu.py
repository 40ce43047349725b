"""What tests/test_gemm_exact_gpu.py and tests/test_attn_exact_gpu.py take for granted about their fixtures, proved in fp64 on
the CPU: the GEMM references are integers below 2^24 (exact in f32 in any summation order), the attention probabilities are
exactly 0 or 1/n, and the stored-dS values and every expected attention output survive a bf16 round trip unchanged.  This is
what makes torch.equal a fair demand of the kernels.  For tests/test_attn_fused_exact_gpu.py, at exactly its (shape, B, seed, tag)
tuples: every fixture output is bf16-exact with and without dropout, dy @ W == dO, every k-tile of the signed permutation feeds every
head slice, the written-down P is the fp64 softmax, the sign fixture's xn has no tie anywhere inside the rstd bound, and
attn_drop_mult is rowops_ref.drop_mult under the combined key."""
import pytest
import torch

from tests import exact_ref as R


@pytest.mark.parametrize("M,N,K", R.gemm_shapes(), ids=lambda v: str(v))
def test_gemm_reference_is_an_integer_below_2_24(M, N, K):
    A, B, ref = R.gemm_ints(M, N, K)
    assert float(A.abs().max()) <= 3 and float(B.abs().max()) <= 3 and bool((A == A.round()).all()) and bool((B == B.round()).all())
    assert bool((ref == ref.round()).all())
    # every partial sum, in any order, is bounded by the sum of the magnitudes
    assert float((A.abs() @ B.abs().T).max()) < 2 ** 24
    assert torch.equal(ref.float().double(), ref)


def test_gemm_epilogue_operands_keep_the_result_exact():
    M, N = R.EPI
    for K in (72, 96, 192):
        prod = R.gemm_ints(M, N, K)[2]
        e = R.gemm_extras(M, N)
        for kw in (dict(alpha=0.5), dict(bias=e["bias"]), dict(bias=e["bias"], relu=True), dict(residual=e["residual"]), dict(c0=e["c0"]),
                   dict(aux=e["aux"], aux_scale=0.5), dict(alpha=0.5, bias=e["bias"], relu=True, residual=e["residual"])):
            want = R.gemm_expected(prod, **kw)
            assert torch.equal(want.float().double(), want) and bool((want * 2 == (want * 2).round()).all())
        assert 0.25 < float((e["aux"] == 0).double().mean()) < 0.6


@pytest.mark.parametrize("kind,n,Lq,Lk,dk,causal", R.attn_fixture_cases(), ids=lambda v: str(v))
def test_attention_fixture_is_dyadic_and_bf16_exact(kind, n, Lq, Lk, dk, causal):
    f = R.attn_fixture(kind, R.ATTN_B, R.ATTN_H, Lq, Lk, dk, causal, n)
    cnt = f.mask.sum(-1)
    # n chosen keys per row (the largest power of two that fits a short causal prefix), inside the causal prefix
    want_cnt = torch.tensor([[max(c for c in (1, 2, 4) if c <= min(n, (q + 1) if causal else Lk)) for q in range(Lq)]] * f.H)
    assert torch.equal(cnt, want_cnt)
    if causal:
        assert not bool((f.mask & (torch.arange(Lk)[None, :] > torch.arange(Lq)[:, None])[None]).any())
    # the first key, the last key and every 32-key block are chosen by some row
    hit = f.mask.any(0).any(0)
    assert bool(hit[0]) and bool(hit[Lk - 1]) and all(bool(hit[b:b + 32].any()) for b in range(0, Lk, 32))
    # probabilities are exactly 0 or 1 / n, and they are the softmax of the fixture's scores
    assert bool(((f.P == 0) | (f.P * cnt[None, ..., None] == 1)).all())
    assert float((f.softmax_fp64() - f.P).abs().max()) < 1e-50
    # ... in f32 as well: the chosen keys of a row share one score, every other visible key is at least 128 below it
    # (exp(-128) is below the smallest f32 denormal), and all scores are integers that f32 holds
    S = f.S if f.bias is None else f.S + f.bias[None]
    if causal:
        S = S.masked_fill((torch.arange(Lk)[None, :] > torch.arange(Lq)[:, None])[None, None], float("-inf"))
    top = torch.where(f.mask[None], S, float("-inf")).amax(-1, keepdim=True)
    assert bool((torch.where(f.mask[None], S, top) == top).all())
    assert float((top - torch.where(f.mask[None], float("-inf"), S)).min()) >= 128
    assert torch.equal(f.S.float().double(), f.S) and float(f.S.abs().max()) < 2 ** 24
    # inputs, stored dS and every output are bf16 numbers
    for name in ("q", "k", "v", "do", "ctx", "dS", "dq", "dk_", "dv", "dbias"):
        x = getattr(f, name)
        assert R.bf16_exact(x), (name, float(x.abs().max()))
    # the fixture is not vacuous
    nz = {name: bool((getattr(f, name) != 0).any()) for name in ("dq", "dk_", "dv", "dbias")}
    assert nz == {"onehot": dict(dq=False, dk_=False, dv=True, dbias=False), "onehot_nobias": dict(dq=False, dk_=False, dv=True, dbias=False),
                  "q0": dict(dq=True, dk_=False, dv=True, dbias=True), "k0": dict(dq=False, dk_=True, dv=True, dbias=True)}[kind]
    assert bool((f.ctx != 0).any())


# ---- attention dropout and the fused attention kernels' fixtures (tests/test_attn_fused_exact_gpu.py) ---------------------------
M32 = 0xFFFFFFFF


def _mix32(x):
    """common.h's finaliser on a Python int"""
    x ^= x >> 16
    x = x * 0x85EBCA6B & M32
    x ^= x >> 13
    x = x * 0xC2B2AE35 & M32
    return x ^ x >> 16


def _unmix32(y):
    """its inverse: both multipliers are odd, and y = x ^ (x >> s) is undone by x = y ^ (y >> s) ^ (y >> 2 s) ^ ..."""
    y ^= y >> 16
    y = y * pow(0xC2B2AE35, -1, 1 << 32) & M32
    y ^= (y >> 13) ^ (y >> 26)
    y = y * pow(0x85EBCA6B, -1, 1 << 32) & M32
    return y ^ y >> 16


def test_attn_drop_mult_is_drop_mult_under_the_combined_key():
    import numpy as np
    from tests import rowops_ref as RR
    assert all(_unmix32(_mix32(v)) == v and int(RR.mix32(np.uint64(v))) == _mix32(v) for v in (0, 1, 0x12345678, 0xDEADBEEF, M32))
    off = np.arange(64 * 64 + 3)
    for seed, tag, slab in ((31, 11, 0), (31, 11, 5), (31, 11, 127), (1234, 7, 23), (0xFFFFFFF0, 0xFFFFFFFF, 0xFFFF)):
        # the key make_drop + drop_slab arrive at, in plain integers ...
        key = _mix32((seed * 0x9E3779B1 + tag * 0x7FEB352D + 0x165667B1) & M32)
        key = _mix32(key ^ ((slab * 0x85EBCA77 + 0x27D4EB2F) & M32))
        # ... is the key make_drop alone arrives at from another seed word (everything in it is invertible): under that seed
        # drop_mult, which tests/test_norm_exact_gpu.py and the GEMM tests hold the kernels to, must give the same multipliers
        seed2 = (_unmix32(key) - tag * 0x7FEB352D - 0x165667B1) * pow(0x9E3779B1, -1, 1 << 32) & M32
        assert _mix32((seed2 * 0x9E3779B1 + tag * 0x7FEB352D + 0x165667B1) & M32) == key
        for p in (0.1, 0.5):
            got = R.attn_drop_mult(seed, tag, p, slab, off)
            assert got.dtype == np.float32 and np.array_equal(got, RR.drop_mult(seed2, tag, p, off))
            # and element by element in plain integers
            for o in (0, 1, 63, 64, 4098):
                want = 0.0 if _mix32((o * 0x9E3779B1 + key) & M32) < int(float(np.float32(p)) * 2 ** 32) else float(np.float32(1) / (np.float32(1) - np.float32(p)))
                assert float(got[o]) == want
            assert abs(float((got == 0).mean()) - p) < 0.03
    # p = 0.5: 0 or 2; slabs differ; the mask tensor is laid out [b, h, q, key] with slab = b H + h and offset q Lk + key
    m = R.attn_drop_mask(31, 11, 0.5, 3, 8, 9, 33)
    assert set(m.unique().tolist()) == {0.0, 2.0} and not torch.equal(m[0, 0], m[0, 1]) and not torch.equal(m[0, 1], m[1, 1])
    assert float(m[2, 5, 7, 30]) == float(R.attn_drop_mult(31, 11, 0.5, 2 * 8 + 5, 7 * 33 + 30))


def test_signed_permutation_feeds_every_head_slice_from_every_k_tile():
    W, pi, sign = R.signed_perm()
    assert W.shape == (512, 512) and bool((W.abs().sum(0) == 1).all()) and bool((W.abs().sum(1) == 1).all())
    assert sorted(pi.tolist()) == list(range(512)) and set(sign.tolist()) == {-1.0, 1.0}
    for t in range(8):
        for h in range(8):
            blk = W[64 * t:64 * t + 64, 64 * h:64 * h + 64]
            assert int(blk.abs().sum()) == 8, (t, h)
    # both signs and more than one 16-byte chunk of a row segment inside a block: a swizzle mismatch between the W and dy reads moves them
    assert len({int(c) // 8 for c in pi[:64] % 64}) > 4 and bool((pi != torch.arange(512)).any())


BWD_CASES = [(kind, n, *c, drop) for c in R.FUSED_SHAPES for kind, n in R.fixtures_for(R.FUSED_DK) for drop in (None, R.FUSED_DROP)]


@pytest.mark.parametrize("kind,n,cross,B,H,Lq,Lk,causal,drop", BWD_CASES, ids=lambda v: str(v))
def test_fused_backward_fixture_is_bf16_exact(kind, n, cross, B, H, Lq, Lk, causal, drop):
    f = R.fused_bwd_fixture(kind, n, cross, B, H, Lq, Lk, causal, drop)
    _check_attn_fixture(f, n, drop)
    for name in ("q", "k", "v", "do", "ctx", "dS", "dq", "dk_", "dv"):
        x = getattr(f, name)
        assert R.bf16_exact(x), (name, float(x.abs().max()))
    assert float(f.dq.abs().max()) <= 50 and float(f.dk_.abs().max()) <= 95
    if min(Lq, Lk) >= 5:  # not vacuous (a row with a single visible key has dS = 0)
        nz = {name: bool((getattr(f, name) != 0).any()) for name in ("dq", "dk_", "dv", "dbias")}
        assert nz == {"onehot": dict(dq=False, dk_=False, dv=True, dbias=False), "q0": dict(dq=True, dk_=False, dv=True, dbias=True),
                      "k0": dict(dq=False, dk_=True, dv=True, dbias=True)}[kind]
    # dS is a multiple of 1/4 and the batch sum stays far below 2^24 quarters: dbias is exact in f32 in any order (slab or atomics)
    assert bool((f.dS * 4 == (f.dS * 4).round()).all()) and float(f.dS.abs().sum(0).max()) * 4 < 2 ** 24
    assert torch.equal(f.dbias.float().double(), f.dbias)
    # the kernel is handed dy and W, not dO: dy @ W gives dO back exactly, one product per element
    W = R.signed_perm()[0]
    dy = R.dy_for(f.do)
    assert dy.shape == (B * Lq, 512) and R.bf16_exact(dy) and torch.equal(dy @ W, R.unheads(f.do))
    assert torch.equal(dy.abs() @ W.abs(), R.unheads(f.do).abs())


def _check_attn_fixture(f, n, drop):
    """what test_attention_fixture_is_dyadic_and_bf16_exact demands of the probabilities, at the fused kernels' shapes"""
    Lq, Lk, causal = f.Lq, f.Lk, f.causal
    cnt = f.mask.sum(-1)
    want_cnt = torch.tensor([[max(c for c in (1, 2, 4) if c <= min(n, (q + 1) if causal else Lk)) for q in range(Lq)]] * f.H)
    assert torch.equal(cnt, want_cnt)
    future = (torch.arange(Lk)[None, :] > torch.arange(Lq)[:, None])
    if causal:
        assert not bool((f.mask & future[None]).any())
    hit = f.mask.any(0).any(0)
    reach = min(Lq, Lk) if causal else Lk
    assert bool(hit[0]) and bool(hit[reach - 1]) and (Lq < 8 or all(bool(hit[b:b + 32].any()) for b in range(0, reach, 32)))
    assert bool(((f.P == 0) | (f.P * cnt[None, ..., None] == 1)).all())
    assert float((f.softmax_fp64() - f.P).abs().max()) == 0.0
    S = f.S + f.bias[None]
    if causal:
        S = S.masked_fill(future[None, None], float("-inf"))
    top = torch.where(f.mask[None], S, float("-inf")).amax(-1, keepdim=True)
    assert bool((torch.where(f.mask[None], S, top) == top).all())
    others = torch.where(f.mask[None], float("-inf"), S)
    assert not bool(torch.isfinite(others).any()) or float((top - others).min()) >= 128
    assert torch.equal(S.float().double(), S) and float(f.S.abs().max()) < 2 ** 24
    assert torch.equal(f.lse, top[..., 0] + cnt[None].double().log())  # the chosen keys' bias is 0: the shared score + log n
    if drop is None:
        assert bool((f.M == 1).all())
    else:
        assert torch.equal(f.M, R.attn_drop_mask(*drop, f.B, f.H, Lq, Lk)) and bool(((f.M == 0) | (f.M == 2)).all())
        kept = f.M[f.mask[None].expand_as(f.M)]
        assert f.B * f.H * Lq < 64 or (bool((kept == 0).any()) and bool((kept == 2).any()))  # the mask bites on chosen keys


FWD_CASES = [(kind, n, *c, drop) for c in R.FUSED_FWD_SHAPES for kind, n in R.FUSED_FWD_KINDS for drop in (None, R.FUSED_DROP)]


@pytest.mark.parametrize("kind,n,cross,B,H,Lq,Lk,causal,drop", FWD_CASES, ids=lambda v: str(v))
def test_fused_forward_fixture_is_exact_at_every_stage(kind, n, cross, B, H, Lq, Lk, causal, drop):
    f = R.fused_fwd_fixture(kind, n, cross, B, H, Lq, Lk, causal, drop)
    inner = 64 * H
    _check_attn_fixture(f, n, drop)
    # the norm: x = sign s_r (f32 numbers), mean(x^2) = s_r^2 exactly, xn = sign gamma
    assert torch.equal(f.x.float().double(), f.x) and torch.equal(f.x.abs(), f.s[:, None].expand_as(f.x)) and set(f.s.tolist()) <= {1.0, 2.0, 4.0}
    assert set(f.gamma.tolist()) <= {1.0, 2.0} and torch.equal(f.xn, f.x.sign() * f.gamma[None]) and R.bf16_exact(f.xn)
    assert float((f.rstd * f.s - 1).abs().max()) < 1e-6
    # the projection: one +-1 per k-tile of 64 columns in every row that is not zeroed, integers of magnitude <= 16
    per_tile = f.w.abs().reshape(f.w.shape[0], 8, 64).sum(-1)
    zero_rows = {"onehot": [], "q0": [(0, inner)], "k0": [] if cross else [(inner, 2 * inner)]}[kind]
    live = torch.ones(f.w.shape[0], dtype=torch.bool)
    for a, b in zero_rows:
        live[a:b] = False
    assert bool((per_tile[live] == 1).all()) and bool((per_tile[~live] == 0).all()) and set(f.w.unique().tolist()) <= {-1.0, 0.0, 1.0}
    assert f.proj.shape == (B * Lq, inner if cross else 3 * inner) and bool((f.proj == f.proj.round()).all()) and float(f.proj.abs().max()) <= 16
    assert float((f.xn.abs() @ f.w.abs().T).max()) <= 16  # every partial sum, in any order
    assert R.bf16_exact(f.proj) and (kind == "q0" and cross or bool((f.proj != 0).any()))
    for name in ("q", "k", "v", "ctx"):
        assert R.bf16_exact(getattr(f, name)), name
    assert torch.equal(f.ctx, (f.P * f.M) @ f.v) and bool((f.ctx != 0).any())
    # every product P M v and every partial sum of them is a multiple of 1/4 below 2^8: exact in f32 in any order
    assert bool((f.Pm * 4 == (f.Pm * 4).round()).all()) and float((f.Pm @ f.v.abs()).max()) < 256


def test_sign_fixture_xn_has_no_tie_anywhere_in_the_rstd_bound():
    """bf16(gamma * (x * rstd)) = sign gamma for EVERY f32 rstd the rstd bound admits (all of them are enumerated: the interval holds
    about a hundred f32 numbers), in the kernel's arithmetic: two f32 multiplies, then one rounding to bf16"""
    import numpy as np
    for s in (1.0, 2.0, 4.0):
        ref = (torch.tensor(s * s, dtype=torch.float64) + 1e-6).rsqrt()
        b = float(R.rstd_bound(ref))
        lo, hi = np.float32(float(ref) - b), np.float32(float(ref) + b)
        lo, hi = np.nextafter(lo, np.float32(0)), np.nextafter(hi, np.float32(8))
        assert float(lo) <= float(ref) - b and float(hi) >= float(ref) + b
        rs, r = [], lo
        while r <= hi:
            rs.append(r)
            r = np.nextafter(r, np.float32(8))
        assert 20 < len(rs) < 400
        r = torch.tensor(np.array(rs, dtype=np.float32))
        for sign in (1.0, -1.0):
            for gamma in (1.0, 2.0):
                x = torch.full_like(r, sign * s)
                y = torch.full_like(r, gamma) * (x * r)
                assert float((y.double().abs() / gamma - 1).abs().max()) < 2.0 ** -10  # far from the tie at 1 - 2^-9 (and 1 + 2^-8)
                assert bool((y.to(torch.bfloat16).double() == sign * gamma).all())


@pytest.mark.parametrize("kind,n,Lq,Lk,dk,causal", [(kind, n, *c) for c in R.ATTN_DROP for kind, n in R.fixtures_for(64)], ids=lambda v: str(v))
def test_unfused_dropout_fixture_is_bf16_exact(kind, n, Lq, Lk, dk, causal):
    f = R.attn_fixture(kind, R.ATTN_B, R.ATTN_H, Lq, Lk, dk, causal, n, 0, R.FUSED_DROP)
    assert torch.equal(f.M, R.attn_drop_mask(*R.FUSED_DROP, R.ATTN_B, R.ATTN_H, Lq, Lk))
    kept = f.M[f.mask[None].expand_as(f.M)]
    assert bool((kept == 0).any()) and bool((kept == 2).any())
    for name in ("ctx", "dS", "dq", "dk_", "dv", "dbias"):
        assert R.bf16_exact(getattr(f, name)), name
    assert bool((f.dv != 0).any()) and bool((f.ctx != 0).any())


def test_mfma_backward_lds_rule_matches_the_shapes_the_comments_name():
    fits = {c: R.mfma_bwd_fits(*c[:3]) for c in R.ATTN_MFMA}
    assert not any(R.mfma_bwd_fits(*c[:3]) for c in R.ATTN_FLASH)
    assert fits[(70, 69, 64, False)] and fits[(70, 153, 64, False)] and fits[(33, 69, 128, False)] and fits[(153, 153, 32, True)]
    assert not fits[(33, 153, 128, False)] and not fits[(153, 153, 64, True)]


def test_bf16_unit_roundoff():
    # the constant the per-element bounds are built from: a correctly rounded bf16 store errs by up to 2^-8 relative (just above a
    # power of two), never more, and a perturbation below 2^-9 relative never changes what is stored
    x = torch.linspace(1.0, 2.0, 200001, dtype=torch.float64)
    rel = ((x.to(torch.bfloat16).double() - x).abs() / x)
    assert 2.0 ** -9 < float(rel.max()) <= R.U8
    assert abs(float(torch.tensor(64.25).to(torch.bfloat16)) - 64.25) == 0.25 == R.U8 * 64
    b = torch.arange(0, 128, dtype=torch.float64) / 128 + 1.0  # every bf16 number of a binade
    assert R.bf16_exact(b) and torch.equal((b * (1 + 0.99 * 2.0 ** -9)).to(torch.bfloat16).double(), b)
    assert torch.equal((b * (1 - 0.99 * 2.0 ** -9)).to(torch.bfloat16).double(), b)
