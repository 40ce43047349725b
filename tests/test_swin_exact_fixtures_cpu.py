"""What tests/test_swin_attn_exact_gpu.py takes for granted about its fixtures, proved in fp64 on the CPU: every expected
probability is 0 or a power of two, the surviving keys of a row share one score and every other key is far enough below it to
vanish in f32, inputs and expected outputs are bf16 numbers, and the plain fp64 softmax reference (and its autograd gradients)
agrees with the constructive expectation to 1e-12.  This is what makes torch.equal a fair demand of the kernels."""
import math

import pytest
import torch

from tests import swin_exact_ref as S

_sm = S.small_cases()
SELECT = [(R, w, s, H, C, "dense") for (dn, R, w, s, H, C) in _sm if dn == "bf16"] + \
         sorted({(R, w, s, H, C, form) for (dn, R, w, s, H, C, form, _m) in S.large_cases()})
ONEHOT = sorted({c[1:] for c in S.onehot_cases()})
REGION = sorted({c[1:] for c in S.region_cases()})
FUSED = [(R, w, s, C) for (R, w, s) in S.FUSED_GEO for C in S.FUSED_C]


def is_pow2_or_zero(P):
    nz = P[P > 0]
    return bool((torch.log2(nz) == torch.log2(nz).round()).all())


def check_forward(f, r):
    assert f.alive_scores_equal
    assert is_pow2_or_zero(f.P) and bool((f.P.sum(-1) == 1).all())
    assert float((r["P"] - f.P).abs().max()) < 1e-12
    assert float((r["ctx"] - f.ctx).abs().max()) < 1e-12 * max(1.0, float(f.ctx.abs().max()))
    assert float((r["lse"] - f.lse).abs().max()) < 1e-12 * max(1.0, float(f.lse.abs().max()))
    # in f32 as well: every key that is not among the survivors is at least 90 below them (exp(-90) < 2^-24 / 64 of the row's sum)
    alive = f.P > 0
    top = torch.where(alive, r["S"], -math.inf).amax(-1, keepdim=True)
    assert float((top - torch.where(alive, -math.inf, r["S"])).min()) >= 90
    for name in ("qkv", "dctx", "ctx"):
        assert S.bf16_exact(getattr(f, name)), name
    # q-hat and k-hat are bf16 numbers (norms are powers of two), V has no zero entry
    assert S.bf16_exact(f.qh) and S.bf16_exact(f.kh) and bool((f.v_w != 0).all())
    assert bool((f.ctx != 0).any())


@pytest.mark.parametrize("R,w,shift,H,C,form", SELECT, ids=lambda v: str(v))
def test_select_fixture_is_dyadic_and_bf16_exact(R, w, shift, H, C, form):
    f = S.swin_fixture("select", S.B_, R, w, shift, H, C, form)
    r = f.reference()
    check_forward(f, r)
    cnt = f.cnt
    assert set(cnt.unique().tolist()) <= {1.0, 2.0, 4.0}
    if w > 2:
        assert bool((cnt > 1).any()) and bool((cnt == 1).any())
    if shift > 0 and form == "dense" and w > 2:
        # a row whose second key lies in another region: 1/2, 1/2 in unshifted windows, 1, 0 where the regions differ
        nch = f.chosen.sum(-1)[None].expand_as(cnt)
        assert bool(((nch == 2) & (cnt == 1)).any()) and bool(((nch == 2) & (cnt == 2)).any())
    for name in ("dqkv", "dS", "dqh", "dkh", "dbias", "dtable"):
        assert S.bf16_exact(getattr(f, name)) or name in ("dbias", "dtable"), name
        assert torch.equal(getattr(f, name).float().double(), getattr(f, name)), name
    assert bool((f.dls == 0).all()) and float(r["dls"].abs().max()) < 1e-12      # sum_j dS_ij = 0 over keys of equal cosine
    assert float((r["dqkv"] - f.dqkv).abs().max()) < 1e-12 * float(f.dqkv.abs().max())
    want = r["dbias"] if form == "dense" else r["dtable"]
    have = f.dbias if form == "dense" else f.dtable
    assert float((want - have).abs().max()) < 1e-12 * max(1.0, float(have.abs().max()))
    if f.v_bias is not None:
        assert float((r["dv_bias"] - f.dv_bias).abs().max()) < 1e-12 * max(1.0, float(f.dv_bias.abs().max()))
        assert bool((f.dv_bias != 0).any()) and torch.equal(f.dv_bias.float().double(), f.dv_bias)
    assert bool((f.dqkv[:, :C] != 0).any()) and bool((f.dqkv[:, C:2 * C] != 0).any()) and bool((f.dbias != 0).any()) or w == 2
    # the first and the last key of the window are chosen by some row
    assert bool(f.chosen[..., 0].any()) and bool(f.chosen[..., -1].any())


@pytest.mark.parametrize("R,w,shift,H,C", REGION, ids=lambda v: str(v))
def test_region_fixture_probabilities_are_one_over_the_region_size(R, w, shift, H, C):
    f = S.swin_fixture("region", S.B_, R, w, shift, H, C)
    r = f.reference(grads=False)
    check_forward(f, r)
    assert bool((f.cos == 0).all())
    want = {4: {4.0, 8.0, 16.0}, 8: {16.0, 32.0, 64.0}}[w]
    assert set(f.cnt.unique().tolist()) == want


@pytest.mark.parametrize("R,w,shift,H,C", sorted({c[1:6] for c in S.REGION_TABLE}) + REGION, ids=lambda v: str(v))
def test_region_fixture_bias_gradients_are_exact_in_f32(R, w, shift, H, C):
    form = "table" if (R, w, shift, H, C) in {c[1:6] for c in S.REGION_TABLE} else "dense"
    f = S.swin_fixture("region", S.B_, R, w, shift, H, C, form)
    r = f.reference()
    check_forward(f, r)
    assert set(f.cnt.unique().tolist()) <= {4.0, 8.0, 16.0, 32.0, 64.0}
    want, have = (r["dtable"], f.dtable) if form == "table" else (r["dbias"], f.dbias)
    assert float((want - have).abs().max()) < 1e-12 * float(have.abs().max())
    # dyadic and short: any f32 summation order gives the same number; and every pair of one region contributes
    assert torch.equal(have.float().double(), have) and torch.equal((f.dS * 2.0 ** 16), (f.dS * 2.0 ** 16).round())
    assert float((f.dS != 0).double().mean()) > 0.2 and bool((f.dls == 0).all())


@pytest.mark.parametrize("R,w,shift,H,C,perm", ONEHOT, ids=lambda v: str(v))
def test_onehot_fixture_selects_by_the_scores_alone(R, w, shift, H, C, perm):
    f = S.swin_fixture("onehot", S.B_, R, w, shift, H, C, perm=perm)
    r = f.reference(grads=False)
    assert bool((f.cnt == 1).all()) and f.bias is not None and bool((f.bias == 0).all())
    n = w * w
    if perm and w > 2:
        assert not torch.equal(f.pi, torch.arange(n))
    assert torch.equal(f.pi.sort().values, torch.arange(n)) and torch.equal(S.bands(w, shift)[f.pi], S.bands(w, shift))
    # the other keys' share of the output is below 2^-24 of a (nonzero) V entry: every other score is ~100 lower
    assert float((r["P"] - f.P).abs().max()) * n < 2.0 ** -30
    assert bool((f.v_w != 0).all()) and S.bf16_exact(f.qkv) and S.bf16_exact(f.ctx)
    assert float((r["ctx"] - f.ctx).abs().max()) < 2.0 ** -24 * float(f.v_w.abs().min())


@pytest.mark.parametrize("R,w,shift,C", FUSED, ids=lambda v: str(v))
def test_fused_operands_reproduce_the_fixture(R, w, shift, C):
    H = C // 32
    for kind in ("select", "onehot"):
        f = S.swin_fixture(kind, S.B_, R, w, shift, H, C, "dense", True)
        x, wq = f.fused_operands()
        assert S.bf16_exact(x) and S.bf16_exact(wq)
        qkv = S.fused_qkv(x, wq, None)
        # q and k differ from the fixture's by the window's power of two (the cosine does not notice), v is the fixture's
        assert torch.equal(qkv[:, 2 * C:], f.qkv[:, 2 * C:])
        r = S.swin_reference(qkv, f.ls, S.B_, R, w, shift, H, C, f.bias)
        tol = 1e-12 if kind == "select" else 2.0 ** -24
        assert float((r["ctx"] - f.ctx).abs().max()) < tol
        bv = torch.cat([torch.zeros(2 * C, dtype=torch.float64), torch.tensor([1.0, -1.0] * (C // 2), dtype=torch.float64)])
        assert S.bf16_exact(f.ctx + bv[2 * C:])    # with a value bias of +-1 the context is the fixture's + the bias


def test_regions_match_the_shift_mask_of_the_oracle():
    from oracle import swin_t5_oracle as O
    for R, w, shift in [(8, 4, 2), (14, 7, 3), (12, 4, 1), (16, 8, 4)]:
        reg = S.region_ids(R, w, shift)
        mask = O.swin_shift_mask(R, w, shift, torch.float64)
        assert torch.equal((reg[:, :, None] != reg[:, None, :]).double() * -100.0, mask)
    x = torch.arange(2 * 9 * 9 * 3, dtype=torch.float64).reshape(2 * 81, 3)
    assert torch.equal(S.to_tokens(S.to_windows(x, 2, 9, 4, 2), 2, 9, 4, 2), x)


def test_f32_logf_of_one_and_expf_of_zero_hold_on_the_reference_side():
    # the exact lse assertion needs log(1) = 0 and exp(0) = 1; the GPU test checks the same of the kernels' __logf / __expf
    assert math.log(1.0) == 0.0 and math.exp(0.0) == 1.0
