"""klab_t5_attn_bwd_fused (o / co projection dgrad -> attention backward of one T5 attention sub-layer in one launch) against the two
launches it replaces (ops.gemm for the dgrad + ops.t5_attn_bwd) on the same inputs, and against fp32 torch."""
import pytest
import torch

from tests.helpers import rel_l2

pytestmark = pytest.mark.gpu

H, DK, D = 8, 64, 512
INNER = H * DK
PAD = 64  # extra columns of every output buffer: must stay untouched


@pytest.fixture(scope="module")
def ops():
    from klab_multimodalmodel_amd import ops as K
    return K


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return torch.randn(*shape, generator=g) * scale


def _ref_grads(q, k, v, bias, causal, dout):
    """fp32 torch: [B, H, L, dk] tensors, returns dq, dk, dv, dbias"""
    q, k, v = (t.clone().requires_grad_(True) for t in (q, k, v))
    b = bias.clone().requires_grad_(True) if bias is not None else None
    s = q @ k.transpose(2, 3)
    if b is not None:
        s = s + b
    if causal:
        Lq, Lk = s.shape[-2:]
        s = s.masked_fill(~torch.tril(torch.ones(Lq, Lk, dtype=torch.bool)), float("-inf"))
    (torch.softmax(s, -1) @ v).backward(dout)
    return q.grad, k.grad, v.grad, (b.grad if b is not None else None)


def _heads(x, B, L):  # [B*L, inner] -> [B, H, L, dk]
    return x[:, :INNER].float().cpu().reshape(B, L, H, DK).transpose(1, 2)


def _rows(x, B, L):  # [B, H, L, dk] -> [B*L, inner]
    return x.transpose(1, 2).reshape(B * L, INNER)


@pytest.mark.parametrize("B,Lq,Lk,causal,cross,drop", [(3, 64, 64, True, False, 0.0), (2, 58, 58, False, False, 0.0), (3, 64, 58, False, True, 0.0),
                                                       (2, 33, 33, True, False, 0.1), (2, 40, 64, False, True, 0.1), (70, 64, 64, True, False, 0.1)])
def test_attn_bwd_fused_matches_the_two_launches(ops, B, Lq, Lk, causal, cross, drop):
    dt = torch.bfloat16
    dev = "cuda"
    sd = torch.tensor([31], dtype=torch.int32, device=dev)
    w = (rnd(D, INNER, seed=1) * D ** -0.5).to(dt).to(dev)  # o / co weight [d_model, inner]
    dy = rnd(B * Lq, D, seed=2).to(dt).to(dev)
    if cross:
        qbuf = rnd(B * Lq, INNER, seed=3, scale=0.5).to(dt).to(dev)
        kvbuf = rnd(B * Lk, 2 * INNER, seed=4, scale=0.5).to(dt).to(dev)
        q, k, v, ldq, ldkv = qbuf, kvbuf[:, :INNER], kvbuf[:, INNER:], INNER, 2 * INNER
    else:
        qbuf = rnd(B * Lq, 3 * INNER, seed=3, scale=0.5).to(dt).to(dev)
        q, k, v, ldq, ldkv = qbuf, qbuf[:, INNER:], qbuf[:, 2 * INNER:], 3 * INNER, 3 * INNER
    bias = None if cross else rnd(H, Lq, Lk, seed=5).to(dev)
    kw = dict(B=B, H=H, Lq=Lq, Lk=Lk, dk=DK, bias=bias, causal=causal, drop_p=drop, seed=sd, tag=11)
    ctx = torch.zeros(B * Lq, INNER, device=dev, dtype=dt)
    lse = torch.empty(B, H, Lq, device=dev)
    ops.t5_attn_fwd(q, k, v, ctx, lse, ldq=ldq, ldk=ldkv, ldv=ldkv, **kw)

    def outputs():
        # q | k | v gradients in the engine's layouts (self: one [rows, 3 inner] buffer; cross: dq + a [rows, 2 inner] k | v buffer),
        # each buffer PAD columns wider and filled with a sentinel
        if cross:
            dqb = torch.full((B * Lq, INNER + PAD), 7.0, device=dev, dtype=dt)
            dkvb = torch.full((B * Lk, 2 * INNER + PAD), 7.0, device=dev, dtype=dt)
            return (dqb, dkvb), dqb, dkvb[:, :INNER], dkvb[:, INNER:]
        dqkv = torch.full((B * Lq, 3 * INNER + PAD), 7.0, device=dev, dtype=dt)
        return (dqkv,), dqkv, dqkv[:, INNER:], dqkv[:, 2 * INNER:]

    ds_shape = B * H * Lq * ((Lk + 31) // 32 * 32)
    # two launches: the dgrad GEMM (as the engine's linear_dgrad) + the attention backward
    bufs0, dq0, dk0, dv0 = outputs()
    dctx = torch.empty(B * Lq, INNER, device=dev, dtype=dt)
    ops.gemm(dy, w, dctx, M=B * Lq, N=INNER, K=D, a_kmajor=True, b_kmajor=False, ldb=INNER)
    dbias0 = torch.zeros(H, Lq, Lk, device=dev) if bias is not None else None
    ds0 = torch.zeros(ds_shape, device=dev, dtype=dt) if bias is not None else None
    ops.t5_attn_bwd(q, k, v, ctx, lse, dctx, dq0, dk0, dv0, dbias=dbias0, ds_ws=ds0, ldq=ldq, ldk=ldkv, ldv=ldkv,
                    lddq=dq0.stride(0), lddk=dk0.stride(0), lddv=dv0.stride(0), **kw)
    # fused
    bufs1, dq1, dk1, dv1 = outputs()
    dbias1 = torch.zeros(H, Lq, Lk, device=dev) if bias is not None else None
    ds1 = torch.full((ds_shape,), 3.0, device=dev, dtype=dt) if bias is not None else None
    ops.t5_attn_bwd_fused(dy, w, q, k, v, ctx, lse, dq1, dk1, dv1, dbias=dbias1, ds_ws=ds1, ldq=ldq, ldk=ldkv, ldv=ldkv, **kw)
    torch.cuda.synchronize()

    sl = (slice(None), slice(0, INNER))
    for a, b_ in ((dq1, dq0), (dk1, dk0), (dv1, dv0)):
        assert rel_l2(a[sl].float().cpu(), b_[sl].float().cpu()) < 8e-3
    for bb in bufs1:
        assert bool((bb[:, -PAD:] == 7.0).all())  # columns outside the head slices untouched
    if bias is not None:
        assert rel_l2(ds1.float().cpu(), ds0.float().cpu()) < 1e-2
        assert rel_l2(dbias1.cpu(), dbias0.cpu()) < 1e-2
    if drop == 0.0:  # against fp32 torch (the tolerances of test_t5_attention_fwd_bwd)
        dout = (dy.float() @ w.float()).cpu()
        rq, rk, rv, rb = _ref_grads(_heads(q, B, Lq), _heads(k, B, Lk), _heads(v, B, Lk), bias.cpu() if bias is not None else None, causal,
                                    _heads(dout, B, Lq))
        t = 2 * 1.5e-2
        assert rel_l2(dq1[sl].float().cpu(), _rows(rq, B, Lq)) < t
        assert rel_l2(dk1[sl].float().cpu(), _rows(rk, B, Lk)) < t
        assert rel_l2(dv1[sl].float().cpu(), _rows(rv, B, Lk)) < t
        if rb is not None:
            assert rel_l2(dbias1.cpu(), rb) < t
    # outside the envelope (d_model 256, or more than 64 keys): the caller keeps the two launches
    with pytest.raises(NotImplementedError):
        ops.t5_attn_bwd_fused(dy[:, :256].contiguous(), w[:256].contiguous(), q, k, v, ctx, lse, dq1, dk1, dv1, ldq=ldq, ldk=ldkv,
                              ldv=ldkv, **kw)
    with pytest.raises(NotImplementedError):
        ops.t5_attn_bwd_fused(dy, w, q, k, v, ctx, lse, dq1, dk1, dv1, ldq=ldq, ldk=ldkv, ldv=ldkv, **dict(kw, Lk=65, bias=None))
