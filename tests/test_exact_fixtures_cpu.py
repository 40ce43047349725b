"""What tests/test_gemm_exact_gpu.py and tests/test_attn_exact_gpu.py take for granted about their fixtures, proved in fp64 on
the CPU: the GEMM references are integers below 2^24 (exact in f32 in any summation order), the attention probabilities are
exactly 0 or 1/n, and the stored-dS values and every expected attention output survive a bf16 round trip unchanged.  This is
what makes torch.equal a fair demand of the kernels."""
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
