"""klab_t5_attn_fwd / klab_t5_attn_bwd in the shape the engine gives the cross-attention of n captions per image: batch B = 2
images, Lq = n*Lt queries on contiguous image-major rows, Lk = Le keys, six heads (tests/multi_caption_shapes.py has the shapes
and why).  Neither entry point bounds Lq: the one-workgroup matrix-core kernels take these shapes while their images fit LDS, the
streaming kernels or the generic ones of attn_t5.hip otherwise, and the f32 kernels loop over 16-query tiles -- so the engine needed
no query-group argument, and there is none to test.

As tests/test_attn_exact_gpu.py: on the dyadic fixtures of tests/exact_ref.py whatever a kernel stores as bf16 equals the fp64
reference bit for bit and f32 outputs stay within 2^-20 relative (16 ulp: one exp, one log, one reciprocal), exact zeros exact; on
randn operands every output element stays within the bound counted from the roundings on its data path.  Outputs sit in the
sentinel-filled buffers of tests/attn_harness.py.  tests/test_multi_caption_cpu.py proves the fixtures exact at these shapes.

The grouped call against the per-caption calls: d k / d v of the B-batch, n*Lt-query call equal the sum over the image's captions,
caption 0 first, of the Lt-query calls on each caption's rows -- on the exact fixtures every partial and the sum are bf16 numbers,
so the equality is one of bits; ctx, lse and d q of a caption's rows are the per-caption call's."""
import pytest
import torch

from tests import exact_ref as R
from tests.attn_harness import FlatOut, MatOut, assert_bf16_equal, assert_f32_close, fused_input, ratio
from tests.multi_caption_shapes import XATTN_B as B, XATTN_H as H, XATTN_SHAPES, caption_slices, xattn_kinds

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "bf16": torch.bfloat16}
CASES = [(dt, *c) for c in XATTN_SHAPES for dt in ("bf16", "f32")]


@pytest.fixture(scope="module")
def ops():
    from klab_multimodalmodel_amd import ops as K
    return K


def assert_out(got, ref, what, mag=None):
    if got.dtype == torch.bfloat16:
        assert_bf16_equal(got, ref, what)
    else:
        assert_f32_close(got, ref, what, mag)


class Cross:
    """device operands of one cross-attention problem in the engine's layout: q alone, k | v side by side (kv_all), ctx | dO"""

    def __init__(self, q, k, v, do, bias, dtype, Lq, Lk, dk):
        self.Lq, self.Lk, self.dk, self.dtype, self.do = Lq, Lk, dk, dtype, do
        self.nb = q.shape[0]
        _qb, self.ldq, (self.q,) = fused_input([q], dtype)
        _kvb, self.ldkv, (self.k, self.v) = fused_input([k, v], dtype)
        self._keep = (_qb, _kvb)
        self.bias = None if bias is None else bias.float().cuda()
        self.kw = dict(B=self.nb, H=H, Lq=Lq, Lk=Lk, dk=dk, bias=self.bias, causal=False, ldq=self.ldq, ldk=self.ldkv, ldv=self.ldkv)

    def forward(self, ops):
        ctx = MatOut(self.nb * self.Lq, H * self.dk, 1, self.dtype, H)
        lse = FlatOut(self.nb * H * self.Lq, torch.float32)
        ops.t5_attn_fwd(self.q, self.k, self.v, ctx.views[0], lse.view, ldo=ctx.ld, **self.kw)
        torch.cuda.synchronize()
        return ctx.fetch(self.Lq)[0], lse.fetch().reshape(self.nb, H, self.Lq)

    def backward(self, ops, ctx, lse):
        """as the engine calls it for cross-attention: no bias gradient.  -> dq [B, H, Lq, dk], dk, dv [B, H, Lk, dk]"""
        _cb, ldc, (cv, dov) = fused_input([ctx, self.do], self.dtype)
        dq = MatOut(self.nb * self.Lq, H * self.dk, 1, self.dtype, H)
        dkv = MatOut(self.nb * self.Lk, H * self.dk, 2, self.dtype, H)
        ops.t5_attn_bwd(self.q, self.k, self.v, cv, lse.float().cuda(), dov, dq.views[0], dkv.views[0], dkv.views[1], ldo=ldc, lddo=ldc,
                        lddq=dq.ld, lddk=dkv.ld, lddv=dkv.ld, **self.kw)
        torch.cuda.synchronize()
        dk_, dv = dkv.fetch(self.Lk)
        return dict(dq=dq.fetch(self.Lq)[0], dk=dk_, dv=dv)


@pytest.mark.parametrize("dtype,Lq,n,Lk,dk", CASES, ids=lambda v: str(v))
def test_exact_fixtures_per_image_and_per_caption(ops, dtype, Lq, n, Lk, dk):
    for kind, nk in xattn_kinds(dk):
        f = R.attn_fixture(kind, B, H, Lq, Lk, dk, False, nk)
        tag = f"{kind} n_keys={nk} (B, H, Lq, Lk, dk) = ({B}, {H}, {Lq}, {Lk}, {dk}) {dtype}"
        pr = Cross(f.q, f.k, f.v, f.do, f.bias, DT[dtype], Lq, Lk, dk)
        ctx, lse = pr.forward(ops)
        assert_out(ctx, f.ctx, f"forward ctx, {tag}")
        assert_f32_close(lse, f.lse, f"forward lse, {tag}")
        absds = f.dS.abs()
        mags = dict(dq=absds @ f.k.abs(), dk=absds.transpose(-1, -2) @ f.q.abs(), dv=f.Pm.transpose(-1, -2) @ f.do.abs())
        got = pr.backward(ops, f.ctx, f.lse)
        for name, ref in (("dq", f.dq), ("dk", f.dk_), ("dv", f.dv)):
            assert_out(got[name], ref, f"backward {name}, {tag}", mags[name])
        # the image's n captions one by one: Lt queries each, the image's keys
        sk, sv = torch.zeros_like(f.dk_), torch.zeros_like(f.dv)
        for j, sl in enumerate(caption_slices(Lq, n)):
            Lt = Lq // n
            cut = lambda x: x[:, :, sl].contiguous()
            pj = Cross(cut(f.q), f.k, f.v, cut(f.do), None if f.bias is None else f.bias[:, sl].contiguous(), DT[dtype], Lt, Lk, dk)
            cj, lj = pj.forward(ops)
            assert_out(cj, cut(f.ctx), f"caption {j}: forward ctx, {tag}")
            assert_f32_close(lj, f.lse[:, :, sl], f"caption {j}: forward lse, {tag}")
            gj = pj.backward(ops, cut(f.ctx), f.lse[:, :, sl].contiguous())
            assert_out(gj["dq"], cut(f.dq), f"caption {j}: backward dq, {tag}", cut(mags["dq"]))
            if dtype == "bf16":  # the grouped call's rows of this caption, bit for bit
                assert torch.equal(cj, ctx[:, :, sl]) and torch.equal(gj["dq"], got["dq"][:, :, sl]), f"caption {j}, {tag}"
            sk += gj["dk"].double()  # caption 0 first; every partial is a bf16 number, the sums are exact in fp64
            sv += gj["dv"].double()
        if dtype == "bf16":
            assert torch.equal(sk, got["dk"].double()) and torch.equal(sv, got["dv"].double()), f"sum over the captions, {tag}"
        else:  # f32 stores: each caption's terms within 2^-20 of their magnitudes, which add up to the image's
            assert_f32_close(sk, f.dk_, f"sum over the captions: dk, {tag}", mags["dk"])
            assert_f32_close(sv, f.dv, f"sum over the captions: dv, {tag}", mags["dv"])


@pytest.mark.parametrize("dtype,Lq,n,Lk,dk", CASES, ids=lambda v: str(v))
def test_random_operands_per_element(ops, dtype, Lq, n, Lk, dk):
    d = R.attn_randn(B, H, Lq, Lk, dk, False, False)
    q, k, v, do = d["q"], d["k"], d["v"], d["do"]
    assert d["bias"] is None
    pr = Cross(q, k, v, do, None, DT[dtype], Lq, Lk, dk)
    ctx, lse = pr.forward(ops)
    f32f = R.attn_f32_factor(q, k, Lk, dk)
    cb = R.attn_f32_bounds(dict(P=d["P"], D=d["P"]), q, k, v, do, Lq, Lk, dk, B)["ctx"] if dtype == "f32" else R.attn_fwd_bound(d["P"], v)
    worst = [ratio(ctx, d["ctx"], cb, "ctx"), ratio(lse, d["lse"], f32f.amax(-1) + 4.0 * R.U24 * d["lse"].abs(), "lse")]
    ctx64, lse64 = ctx.double(), lse.double()  # the backward is a function of what the forward left behind
    r = R.attn_backward_reference(q, k, v, None, False, ctx64, lse64, do)
    got = pr.backward(ops, ctx64, lse64)
    bnd = R.attn_f32_bounds(r, q, k, v, do, Lq, Lk, dk, B) if dtype == "f32" else R.attn_bwd_bounds(r, q, k, v, do, Lq, Lk, dk, B, stored_ds=False)
    for name in ("dq", "dk", "dv"):
        worst.append(ratio(got[name], r[name], bnd[name], name))
    print(f"\ncross-attention randn {dtype} (Lq, Lk, dk) = ({Lq}, {Lk}, {dk}): worst err / bound", [round(float(x), 3) for x, _m in worst])
    bad = [msg for v_, msg in worst if not v_ <= 1.0]
    assert not bad, bad
