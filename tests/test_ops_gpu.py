"""GPU parity of every C-ABI kernel against the CPU oracle / a plain fp32 torch reference.

All calls go through libklab_mm.so (ctypes).  fp32 kernels: rel-L2 <= 2e-5; bf16 kernels (bf16
operands, fp32 accumulate): rel-L2 <= 1.5e-2 against an fp32 reference fed the same bf16-rounded inputs.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import swin_t5_oracle as O
from tests.helpers import rel_l2

pytestmark = pytest.mark.gpu

DT = [torch.float32, torch.bfloat16]


def tol(dt):
    return 2e-5 if dt == torch.float32 else 1.5e-2


@pytest.fixture(scope="module")
def ops():
    from klab_multimodalmodel_amd import ops as K
    return K


def dev(t, dt=None):
    t = t.cuda()
    return t.to(dt) if dt is not None else t


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return torch.randn(*shape, generator=g) * scale


def seed_word(v=1234):
    return torch.tensor([v], dtype=torch.int32).cuda()


# ------------------------------------------------------------------------------------------ GEMM
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("M,N,K", [(21, 24, 16), (64, 64, 64), (100, 136, 72), (384, 512, 512), (2048, 2048, 256), (130, 32128 // 8, 128)])
def test_gemm_nt_epilogues(ops, dt, M, N, K):
    A, B = rnd(M, K, seed=1).to(dt), rnd(N, K, seed=2).to(dt)
    bias = rnd(N, seed=3)
    res = rnd(M, N, seed=4)
    ref = A.float() @ B.float().t()
    # plain, f32 out
    Cf = torch.empty(M, N, device="cuda")
    ops.gemm(dev(A), dev(B), Cf, M=M, N=N, K=K)
    assert rel_l2(Cf.cpu(), ref) < tol(dt)
    # alpha + bias + relu + residual, dtype out
    Ct = torch.empty(M, N, device="cuda", dtype=dt)
    ops.gemm(dev(A), dev(B), Ct, M=M, N=N, K=K, alpha=0.5, bias=dev(bias), act=1, residual=dev(res))
    assert rel_l2(Ct.float().cpu(), F.relu(0.5 * ref + bias) + res) < tol(dt) * 1.5
    # gelu, residual in dtype, accumulate into f32
    Cf.fill_(1.0)
    ops.gemm(dev(A), dev(B), Cf, M=M, N=N, K=K, bias=dev(bias), act=2, residual=dev(res.to(dt)), accumulate=True)
    assert rel_l2(Cf.cpu(), F.gelu(ref + bias) + res.to(dt).float() + 1.0) < tol(dt) * 1.5


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("M,N,K", [(24, 40, 16), (96, 64, 40), (512, 128, 256), (2048, 2048, 264)])
def test_gemm_nn_tn_layouts(ops, dt, M, N, K):
    # dgrad form: dX[M,N] = dY[M,K] @ W[K,N]   (B stored m-major: B(n,k) = W[k*ldw + n])
    dY, W = rnd(M, K, seed=5).to(dt), rnd(K, N, seed=6).to(dt)
    C1 = torch.empty(M, N, device="cuda")
    ops.gemm(dev(dY), dev(W), C1, M=M, N=N, K=K, b_kmajor=False)
    assert rel_l2(C1.cpu(), dY.float() @ W.float()) < tol(dt)
    # wgrad form: dW[M,N] = dY[K,M]^T @ X[K,N]   (both m-major, contraction over the slow dim)
    dY2, X = rnd(K, M, seed=7).to(dt), rnd(K, N, seed=8).to(dt)
    C2 = torch.empty(M, N, device="cuda")
    ops.gemm(dev(dY2), dev(X), C2, M=M, N=N, K=K, a_kmajor=False, b_kmajor=False)
    assert rel_l2(C2.cpu(), dY2.float().t() @ X.float()) < tol(dt)
    # a m-major, b k-major
    Bk = rnd(N, K, seed=9).to(dt)
    C3 = torch.empty(M, N, device="cuda", dtype=dt)
    ops.gemm(dev(dY2), dev(Bk), C3, M=M, N=N, K=K, a_kmajor=False)
    assert rel_l2(C3.float().cpu(), dY2.float().t() @ Bk.float().t()) < tol(dt) * 1.5


@pytest.mark.parametrize("dt", DT)
def test_gemm_wgrad_ragged_contraction(ops, dt):
    # contraction over B*L = 21 rows (tiny decoder batch): any K is legal when both operands are m-major
    K, M, N = 21, 128, 64
    dY, X = rnd(K, M, seed=7).to(dt), rnd(K, N, seed=8).to(dt)
    C2 = torch.empty(M, N, device="cuda")
    ops.gemm(dev(dY), dev(X), C2, M=M, N=N, K=K, a_kmajor=False, b_kmajor=False)
    assert rel_l2(C2.cpu(), dY.float().t() @ X.float()) < tol(dt)
    with pytest.raises(NotImplementedError):  # feature dims must be multiples of the 16-byte vector
        ops.gemm(dev(dY), dev(X), C2, M=21, N=N, K=K, a_kmajor=False, b_kmajor=False)


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("M,N,K", [(512, 512, 4096), (128, 64, 3712), (64, 64, 2048), (1536, 512, 4096)])
def test_gemm_wgrad_split_k_atomics(ops, dt, M, N, K):
    # small outputs + long contraction: the kernel splits K over workgroups and adds partials with f32 atomics
    dY, X = rnd(K, M, seed=7).to(dt), rnd(K, N, seed=8).to(dt)
    C2 = torch.full((M, N), 0.5, device="cuda")
    ops.gemm(dev(dY), dev(X), C2, M=M, N=N, K=K, a_kmajor=False, b_kmajor=False, accumulate=True, atomic_ok=True)
    assert rel_l2(C2.cpu(), dY.float().t() @ X.float() + 0.5) < tol(dt)


# the 256 x 256 eight-wave kernel (csrc/mm8p.hip), forced through name_tag=2: all four operand layouts, ragged M / N edges, an odd
# number of k-tiles, every epilogue family, C += and the split-K atomic form -- against fp32 torch on the same bf16 operands
@pytest.mark.parametrize("M,N,K", [(256, 256, 128), (512, 768, 192), (4896, 1024, 1024), (1000, 520, 320), (304, 264, 4096), (2048, 4096, 1088)])
@pytest.mark.parametrize("ak,bk", [(True, True), (True, False), (False, False), (False, True)])
def test_gemm_large_tile_kernel_layouts(ops, M, N, K, ak, bk):
    dt = torch.bfloat16
    A = rnd(*((M, K) if ak else (K, M)), seed=11).to(dt)
    B = rnd(*((N, K) if bk else (K, N)), seed=12).to(dt)
    ref = (A.float() if ak else A.float().t()) @ (B.float().t() if bk else B.float())
    C = torch.full((M, N), 7.0, device="cuda")
    ops.gemm(dev(A), dev(B), C, M=M, N=N, K=K, a_kmajor=ak, b_kmajor=bk, name_tag=2)
    assert rel_l2(C.cpu(), ref) < 2e-3, rel_l2(C.cpu(), ref)  # (bf16 operands, fp32 accumulation: only the summation order differs)
    Cb = torch.empty(M, N, device="cuda", dtype=dt)
    ops.gemm(dev(A), dev(B), Cb, M=M, N=N, K=K, a_kmajor=ak, b_kmajor=bk, name_tag=2)
    assert rel_l2(Cb.float().cpu(), ref) < 4e-3
    Cs = torch.empty(M, N, device="cuda", dtype=dt)
    ops.gemm(dev(A), dev(B), Cs, M=M, N=N, K=K, a_kmajor=ak, b_kmajor=bk, name_tag=3)  # the four-wave ring on the same operands
    assert rel_l2(Cb.float().cpu(), Cs.float().cpu()) < 4e-3


@pytest.mark.parametrize("M,N,K", [(512, 512, 256), (700, 392, 1024)])
def test_gemm_large_tile_kernel_epilogues(ops, M, N, K):
    dt = torch.bfloat16
    A, B = rnd(M, K, seed=1).to(dt), rnd(N, K, seed=2).to(dt)
    bias, res = rnd(N, seed=3), rnd(M, N, seed=4)
    ref = A.float() @ B.float().t()
    kw = dict(M=M, N=N, K=K, name_tag=2)
    Ct = torch.empty(M, N, device="cuda", dtype=dt)
    ops.gemm(dev(A), dev(B), Ct, alpha=0.5, bias=dev(bias), act=1, residual=dev(res), **kw)
    assert rel_l2(Ct.float().cpu(), F.relu(0.5 * ref + bias) + res) < tol(dt) * 1.5
    Cf = torch.full((M, N), 1.0, device="cuda")
    ops.gemm(dev(A), dev(B), Cf, bias=dev(bias), act=2, residual=dev(res.to(dt)), accumulate=True, **kw)
    assert rel_l2(Cf.cpu(), F.gelu(ref + bias) + res.to(dt).float() + 1.0) < tol(dt) * 1.5
    Cf2 = torch.empty(M, N, device="cuda")
    ops.gemm(dev(A), dev(B), Cf2, residual=dev(res), **kw)  # the T5 sub-layer output form: f32 residual stream
    assert rel_l2(Cf2.cpu(), ref + res) < tol(dt)
    aux = rnd(M, N, seed=5)
    aux[aux.abs() < 0.5] = 0
    aux = aux.to(dt)
    Ca = torch.empty(M, N, device="cuda", dtype=dt)
    ops.gemm(dev(A), dev(B), Ca, aux=dev(aux), aux_mode=1, aux_scale=1.25, **kw)  # relu-mask dgrad form
    assert rel_l2(Ca.float().cpu(), torch.where(aux.float() != 0, ref * 1.25, torch.zeros(()))) < tol(dt)
    z = aux.float().clone().requires_grad_(True)
    F.gelu(z).sum().backward()
    ops.gemm(dev(A), dev(B), Ca, aux=dev(aux), aux_mode=2, **kw)
    assert rel_l2(Ca.float().cpu(), ref * z.grad) < tol(dt) * 2
    # dropout: the same mask as the four-wave kernels produce for (seed, tag, element index)
    sd = seed_word(77)
    Cd, Cd2 = torch.empty(M, N, device="cuda", dtype=dt), torch.empty(M, N, device="cuda", dtype=dt)
    ops.gemm(dev(A), dev(B), Cd, act=1, drop_p=0.25, seed=sd, tag=5, **kw)
    ops.gemm(dev(A), dev(B), Cd2, act=1, drop_p=0.25, seed=sd, tag=5, M=M, N=N, K=K, name_tag=3)
    assert bool(((Cd == 0) == (Cd2 == 0)).all()) and rel_l2(Cd.float().cpu(), Cd2.float().cpu()) < 4e-3


@pytest.mark.parametrize("M,N,K", [(512, 512, 4096), (256, 256, 32128 // 2 // 64 * 64), (1536, 512, 4096)])
def test_gemm_large_tile_kernel_split_k(ops, M, N, K):
    dt = torch.bfloat16
    dY, X = rnd(K, M, seed=7).to(dt), rnd(K, N, seed=8).to(dt)
    C2 = torch.full((M, N), 0.5, device="cuda")
    ops.gemm(dev(dY), dev(X), C2, M=M, N=N, K=K, a_kmajor=False, b_kmajor=False, accumulate=True, atomic_ok=True, name_tag=2)
    assert rel_l2(C2.cpu(), dY.float().t() @ X.float() + 0.5) < 2e-3
    A, W = rnd(M, K, seed=9).to(dt), rnd(K, N, seed=10).to(dt)  # the LM-head dgrad form: long K-major A, m-major B
    C3 = torch.zeros(M, N, device="cuda")
    ops.gemm(dev(A), dev(W), C3, M=M, N=N, K=K, b_kmajor=False, accumulate=True, atomic_ok=True, alpha=0.5, name_tag=2)
    assert rel_l2(C3.cpu(), 0.5 * (A.float() @ W.float())) < 2e-3


@pytest.mark.parametrize("dt", DT)
def test_lmhead_symbol_matches_generic_gemm(ops, dt):
    M, N, K = 256, 1024, 128
    A, B = rnd(M, K, seed=1).to(dt), rnd(N, K, seed=2).to(dt)
    C1 = torch.empty(M, N, device="cuda", dtype=dt)
    C2 = torch.empty(M, N, device="cuda", dtype=dt)
    ops.gemm(dev(A), dev(B), C1, M=M, N=N, K=K, alpha=0.25)
    ops.gemm(dev(A), dev(B), C2, M=M, N=N, K=K, alpha=0.25, name_tag=1)
    assert rel_l2(C1.float().cpu(), C2.float().cpu()) < (1e-6 if dt == torch.float32 else 4e-3)  # k-tile rotation differs with the tile shape


@pytest.mark.parametrize("M,N", [(4096, 32128), (1024, 8192), (1100, 8200), (2048, 64 * 128 + 8)])
def test_lmhead_a_stationary_kernel_matches_fp32(ops, M, N):
    """d_model = 512 logits GEMM, A-stationary form (csrc/lmhead_areg.hip: A fragments in registers, B streamed through a 14-slot
    LDS-DMA ring): every element against an fp32 product of the bf16 operands -- full BASELINE size, ragged row blocks and a ragged
    last column tile, alpha both as a host scalar and as a device scalar (the engine passes d_model^-0.5, HF/t5:1044-1045)."""
    K = 512
    g = torch.Generator().manual_seed(5)
    A = (torch.randn(M, K, generator=g)).to(torch.bfloat16)
    B = (torch.randn(N, K, generator=g)).to(torch.bfloat16)
    C = torch.full((M + 1, N), 3.0, device="cuda", dtype=torch.bfloat16)  # one guard row
    ad = torch.tensor([0.5], device="cuda")
    Ad, Bd = dev(A), dev(B)
    ops.gemm(Ad, Bd, C[:M], M=M, N=N, K=K, alpha=K ** -0.5, alpha_dev=ad, name_tag=1)
    ref = (Ad.float() @ Bd.float().T) * (0.5 * K ** -0.5)
    err = (C[:M].float() - ref).abs().max().item()
    assert err <= 2e-2 * ref.abs().max().item(), err      # bf16 rounding of the output
    assert rel_l2(C[:M].float(), ref) < 3e-3
    assert bool((C[M:] == 3.0).all())
    # the same product through the tiled kernel (the A-stationary form switched off per call is not possible: compare with tag 0)
    C0 = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
    ops.gemm(Ad, Bd, C0, M=M, N=N, K=K, alpha=K ** -0.5, alpha_dev=ad)
    assert rel_l2(C[:M].float(), C0.float()) < 3e-3


@pytest.mark.parametrize("dt", DT)
def test_gemm_aux_modes_and_alpha_dev(ops, dt):
    M, N, K = 72, 48, 32
    A, B = rnd(M, K, seed=1).to(dt), rnd(N, K, seed=2).to(dt)
    aux = rnd(M, N, seed=3)
    aux[aux.abs() < 0.5] = 0
    aux = aux.to(dt)
    ref = A.float() @ B.float().t()
    ad = torch.tensor([0.25], device="cuda")
    C1 = torch.empty(M, N, device="cuda")
    ops.gemm(dev(A), dev(B), C1, M=M, N=N, K=K, aux=dev(aux), aux_mode=1, aux_scale=1.25, alpha_dev=ad)
    assert rel_l2(C1.cpu(), torch.where(aux.float() != 0, 0.25 * ref * 1.25, torch.zeros(()))) < tol(dt)
    z = aux.float().clone().requires_grad_(True)
    F.gelu(z).sum().backward()
    C2 = torch.empty(M, N, device="cuda")
    ops.gemm(dev(A), dev(B), C2, M=M, N=N, K=K, aux=dev(aux), aux_mode=2)
    assert rel_l2(C2.cpu(), ref * z.grad) < tol(dt) * 2


def test_dropout_mask_consistency_and_rate(ops):
    # GEMM-epilogue dropout and the mask regenerated by rmsnorm_bwd (dxt) must be the same function
    M, N, K, p = 512, 256, 32, 0.1
    A = torch.full((M, K), 1.0 / K).cuda()
    B = torch.ones(N, K).cuda()
    sd = seed_word(77)
    Cd = torch.empty(M, N, device="cuda")
    ops.gemm(A, B, Cd, M=M, N=N, K=K, drop_p=p, seed=sd, tag=5)
    keep = (Cd != 0)
    rate = keep.float().mean().item()
    assert abs(rate - (1 - p)) < 0.01
    assert torch.allclose(Cd[keep], torch.tensor(1 / (1 - p), device="cuda"), rtol=1e-5)
    x = torch.randn(M, N, device="cuda")
    w = torch.ones(N, device="cuda")
    rstd = torch.ones(M, device="cuda")
    dxt = torch.empty(M, N, device="cuda")
    ops.rmsnorm_bwd(torch.zeros(M, N, device="cuda"), x, w, rstd, dres=torch.ones(M, N, device="cuda"), dxt=dxt,
                    p_prev=p, tag_prev=5, seed=sd)
    assert torch.equal(dxt != 0, keep)
    # different tag or seed => different mask
    ops.gemm(A, B, Cd, M=M, N=N, K=K, drop_p=p, seed=sd, tag=6)
    assert not torch.equal(Cd != 0, keep)
    ops.gemm(A, B, Cd, M=M, N=N, K=K, drop_p=p, seed=seed_word(78), tag=5)
    assert not torch.equal(Cd != 0, keep)


# ------------------------------------------------------------------------------------------ norms
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("rows,d", [(21, 128), (300, 512), (64, 1024)])
def test_rmsnorm_fwd_bwd(ops, dt, rows, d):
    x, w = rnd(rows, d, seed=1, scale=2.0), 1 + 0.1 * rnd(d, seed=2)
    dy, dres = rnd(rows, d, seed=3), rnd(rows, d, seed=4)
    xr = x.clone().requires_grad_(True)
    wr = w.clone().requires_grad_(True)
    y = O.t5_rmsnorm(xr, wr, 1e-6)
    y.backward(dy)
    yk = torch.empty(rows, d, device="cuda", dtype=dt)
    rstd = torch.empty(rows, device="cuda")
    ops.rmsnorm_fwd(dev(x), dev(w), y=yk, rstd=rstd)
    assert rel_l2(yk.float().cpu(), y.detach()) < (1e-6 if dt == torch.float32 else 4e-3)
    dx = torch.empty(rows, d, device="cuda")
    dxt = torch.empty(rows, d, device="cuda", dtype=dt)
    dw = torch.zeros(d, device="cuda")
    ops.rmsnorm_bwd(dev(dy), dev(x), dev(w), rstd, dres=dev(dres), dx=dx, dxt=dxt, dw=dw)
    assert rel_l2(dx.cpu(), xr.grad + dres) < 1e-5
    assert rel_l2(dxt.float().cpu(), xr.grad + dres) < (1e-5 if dt == torch.float32 else 4e-3)
    assert rel_l2(dw.cpu(), wr.grad) < 1e-5


def test_rmsnorm_row_remap(ops):
    B, G, d, Le, off = 3, 5, 64, 12, 7
    x, w = rnd(B * G, d, seed=1), torch.ones(d)
    out = torch.zeros(B * Le, d, device="cuda")
    ops.rmsnorm_fwd(dev(x), dev(w), y_f32=out, grp=G, grp_stride=Le, off=off)
    ref = O.t5_rmsnorm(x, w, 1e-6).view(B, G, d)
    got = out.view(B, Le, d).cpu()
    assert rel_l2(got[:, off:off + G], ref) < 1e-6
    assert float(got[:, :off].abs().max()) == 0.0


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("rows,C", [(48, 16), (200, 64), (64, 512), (1000, 96), (333, 384), (70, 768), (257, 1024), (40, 1536)])
def test_layernorm_fwd_bwd(ops, dt, rows, C):
    y, g, b = rnd(rows, C, seed=1).to(dt), 1 + 0.1 * rnd(C, seed=2), 0.1 * rnd(C, seed=3)
    sc, dout = rnd(rows, C, seed=4), rnd(rows, C, seed=5)
    yr = y.float().clone().requires_grad_(True)
    gr, br = g.clone().requires_grad_(True), b.clone().requires_grad_(True)
    ref = sc + F.layer_norm(yr, (C,), gr, br, 1e-5)
    ref.backward(dout)
    out = torch.empty(rows, C, device="cuda")
    outt = torch.empty(rows, C, device="cuda", dtype=dt)
    mean, rstd = torch.empty(rows, device="cuda"), torch.empty(rows, device="cuda")
    ops.layernorm_fwd(dev(y), dev(g), dev(b), shortcut=dev(sc), out=out, outt=outt, mean=mean, rstd=rstd)
    assert rel_l2(out.cpu(), ref.detach()) < 2e-6
    assert rel_l2(outt.float().cpu(), ref.detach()) < (2e-6 if dt == torch.float32 else 4e-3)
    dy = torch.empty(rows, C, device="cuda", dtype=dt)
    dg, db = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
    ops.layernorm_bwd(dev(dout), dev(y), dev(g), mean, rstd, dy=dy, dgamma=dg, dbeta=db)
    assert rel_l2(dy.float().cpu(), yr.grad) < (1e-5 if dt == torch.float32 else 5e-3)
    assert rel_l2(dg.cpu(), gr.grad) < 1e-5
    assert rel_l2(db.cpu(), br.grad) < 1e-5
    # the form that also accumulates the column sums of dy (the bias gradient of the Linear in front of the norm), on top of a
    # non-zero buffer; C = 1536 takes the three-kernel path behind the same entry point
    dy2 = torch.empty(rows, C, device="cuda", dtype=dt)
    dg2, db2, dp = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda"), torch.full((C,), 0.5, device="cuda")
    ops.layernorm_bwd(dev(dout), dev(y), dev(g), mean, rstd, dy=dy2, dgamma=dg2, dbeta=db2, dprev_bias=dp)
    assert rel_l2(dy2.float().cpu(), yr.grad) < (1e-5 if dt == torch.float32 else 5e-3)
    assert rel_l2(dg2.cpu(), gr.grad) < 1e-5 and rel_l2(db2.cpu(), br.grad) < 1e-5
    want = 0.5 + yr.grad.sum(0)  # (dy sums to ~0 along a row, not along a column)
    assert float((dp.cpu() - want).abs().max()) <= (1e-4 if dt == torch.float32 else 2e-2) * float(want.abs().max() + 1)


# ------------------------------------------------------------------------------------------ T5 attention
def _attn_ref(q, k, v, bias, causal):
    s = q @ k.transpose(2, 3)
    if bias is not None:
        s = s + bias
    if causal:
        Lq, Lk = s.shape[-2:]
        s = s.masked_fill(~torch.tril(torch.ones(Lq, Lk, dtype=torch.bool)), float("-inf"))
    return F.softmax(s, -1) @ v


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("B,H,Lq,Lk,dk,causal,use_bias", [(2, 4, 7, 7, 16, True, True), (3, 2, 40, 69, 32, False, False), (3, 2, 20, 20, 32, True, True),
                                                          (2, 8, 58, 58, 64, False, True), (2, 8, 64, 64, 64, True, True),
                                                          (1, 2, 33, 153, 64, False, False), (2, 16, 64, 153, 64, False, False),
                                                          (1, 2, 153, 153, 64, False, True), (1, 1, 20, 200, 64, False, True)])
def test_t5_attention_fwd_bwd(ops, dt, B, H, Lq, Lk, dk, causal, use_bias):
    inner = H * dk
    # fused layouts: q in a [B*Lq, 3*inner] buffer, k/v in a [B*Lk, 2*inner] buffer (as the engine uses them)
    qbuf = rnd(B * Lq, 3 * inner, seed=1, scale=0.5).to(dt)
    kvbuf = rnd(B * Lk, 2 * inner, seed=2, scale=0.5).to(dt)
    bias = rnd(H, Lq, Lk, seed=3) if use_bias else None
    dctx = rnd(B * Lq, inner, seed=4).to(dt)
    q = qbuf[:, :inner].float().view(B, Lq, H, dk).transpose(1, 2).clone().requires_grad_(True)
    k = kvbuf[:, :inner].float().view(B, Lk, H, dk).transpose(1, 2).clone().requires_grad_(True)
    v = kvbuf[:, inner:].float().view(B, Lk, H, dk).transpose(1, 2).clone().requires_grad_(True)
    bref = bias.clone().requires_grad_(True) if use_bias else None
    ref = _attn_ref(q, k, v, bref, causal)
    ref.backward(dctx.float().view(B, Lq, H, dk).transpose(1, 2))
    refo = ref.detach().transpose(1, 2).reshape(B * Lq, inner)

    qd, kvd = dev(qbuf), dev(kvbuf)
    ctx = torch.zeros(B * Lq, inner, device="cuda", dtype=dt)
    lse = torch.empty(B, H, Lq, device="cuda")
    kw = dict(B=B, H=H, Lq=Lq, Lk=Lk, dk=dk, bias=dev(bias) if use_bias else None, causal=causal)
    kview, vview = kvd[:, :inner], kvd[:, inner:]
    ops.t5_attn_fwd(qd, kview, vview, ctx, lse, ldq=3 * inner, ldk=2 * inner, ldv=2 * inner, **kw)
    assert rel_l2(ctx.float().cpu(), refo) < tol(dt)
    dqb = torch.zeros(B * Lq, 3 * inner, device="cuda", dtype=dt)
    dkvb = torch.zeros(B * Lk, 2 * inner, device="cuda", dtype=dt)
    dbias = torch.zeros(H, Lq, Lk, device="cuda") if use_bias else None
    # stored-dS + batch-reduction form of the bias gradient (bf16 kernels); B=2 rows of the atomics form stay covered by B=3
    ds_ws = torch.empty(B * H * Lq * ((Lk + 31) // 32 * 32), device="cuda", dtype=dt) if (use_bias and B != 3) else None
    # (fp32 parity mode at Lk > 128, dk = 64 -- T5-large's cross-attention, BASELINE configs[4] -- visits the keys in chunks)
    ops.t5_attn_bwd(qd, kview, vview, ctx, lse, dev(dctx), dqb, dkvb[:, :inner], dkvb[:, inner:], dbias=dbias, ds_ws=ds_ws,
                    ldq=3 * inner, ldk=2 * inner, ldv=2 * inner, lddq=3 * inner, lddk=2 * inner, lddv=2 * inner, **kw)
    t = tol(dt) * 2
    assert rel_l2(dqb[:, :inner].float().cpu(), q.grad.transpose(1, 2).reshape(B * Lq, inner)) < t
    assert rel_l2(dkvb[:, :inner].float().cpu(), k.grad.transpose(1, 2).reshape(B * Lk, inner)) < t
    assert rel_l2(dkvb[:, inner:].float().cpu(), v.grad.transpose(1, 2).reshape(B * Lk, inner)) < t
    assert float(dqb[:, inner:].abs().max()) == 0.0  # untouched columns
    if use_bias:
        assert rel_l2(dbias.cpu(), bref.grad) < t


@pytest.mark.parametrize("B,Lq,Lk,causal,cross,drop", [(3, 64, 64, True, False, 0.0), (2, 58, 58, False, False, 0.0), (3, 64, 58, False, True, 0.0),
                                                       (2, 33, 33, True, False, 0.1), (2, 40, 64, False, True, 0.1), (70, 64, 64, True, False, 0.1)])
def test_t5_attention_sublayer_fused_matches_the_three_launches(ops, B, Lq, Lk, causal, cross, drop):
    """klab_t5_attn_fused_fwd (T5LayerNorm -> q|k|v / q projection -> attention in one launch, HF/t5:59-72 + 206-209 + 144-173) against
    the three launches it replaces on the same inputs: the same normalised rows and 1/rms (same arithmetic, last-bit differences), identical dropout
    masks (same indices), projections / context / log-sum-exp equal up to the projection's summation order; and the projection
    against fp32 torch."""
    dt = torch.bfloat16
    H, dk, d = 8, 64, 512
    inner = H * dk
    x = dev(rnd(B * Lq, d, seed=1, scale=2.0))
    gamma = dev(1 + 0.2 * rnd(d, seed=2))
    nproj = inner if cross else 3 * inner
    w = dev((rnd(nproj, d, seed=3) * d ** -0.5).to(dt))
    bias = None if cross else dev(rnd(H, Lq, Lk, seed=4))
    kv = dev(rnd(B * Lk, 2 * inner, seed=5, scale=0.5).to(dt)) if cross else None
    sd = seed_word(99)
    # reference: the three launches
    xn0 = torch.empty(B * Lq, d, device="cuda", dtype=dt)
    r0 = torch.empty(B * Lq, device="cuda")
    ops.rmsnorm_fwd(x, gamma, y=xn0, rstd=r0)
    p0 = torch.empty(B * Lq, nproj, device="cuda", dtype=dt)
    ops.gemm(xn0, w, p0, M=B * Lq, N=nproj, K=d)
    c0 = torch.zeros(B * Lq, inner, device="cuda", dtype=dt)
    l0 = torch.empty(B, H, Lq, device="cuda")
    kw = dict(B=B, H=H, Lq=Lq, Lk=Lk, dk=dk, bias=bias, causal=causal, drop_p=drop, seed=sd, tag=7)
    if cross:
        ops.t5_attn_fwd(p0, kv[:, :inner], kv[:, inner:], c0, l0, ldq=inner, ldk=2 * inner, ldv=2 * inner, **kw)
    else:
        ops.t5_attn_fwd(p0, p0[:, inner:], p0[:, 2 * inner:], c0, l0, ldq=3 * inner, ldk=3 * inner, ldv=3 * inner, **kw)
    # fused
    xn1 = torch.full((B * Lq, d), 7.0, device="cuda", dtype=dt)
    r1 = torch.zeros(B * Lq, device="cuda")
    p1 = torch.full((B * Lq, nproj), 7.0, device="cuda", dtype=dt)
    c1 = torch.zeros(B * Lq, inner, device="cuda", dtype=dt)
    l1 = torch.empty(B, H, Lq, device="cuda")
    ops.t5_attn_fused_fwd(x, gamma, w, xn1, r1, p1, c1, l1, cross=cross, k=kv[:, :inner] if cross else None, v=kv[:, inner:] if cross else None,
                          ldk=2 * inner if cross else None, ldv=2 * inner if cross else None, **kw)
    # the same arithmetic, but hipcc contracts the multiplies of the two kernels differently: last-bit differences of 1/rms, i.e. a
    # bf16 rounding flip in a fraction of a percent of the elements
    assert rel_l2(r1.cpu(), r0.cpu()) < 1e-6 and rel_l2(xn1.float().cpu(), xn0.float().cpu()) < 1e-3
    assert float((xn1 != xn0).float().mean()) < 5e-2
    ref = xn1.float().cpu() @ w.float().cpu().t()  # the projection of the rows the fused kernel itself normalised
    assert rel_l2(p1.float().cpu(), ref) < 4e-3 and rel_l2(p1.float().cpu(), p0.float().cpu()) < 8e-3
    assert rel_l2(l1.cpu(), l0.cpu()) < 2e-3
    if drop > 0:  # same mask: an output element is exactly zero in one iff ... (masks act on probabilities, compare the contexts loosely)
        assert rel_l2(c1.float().cpu(), c0.float().cpu()) < 3e-2
    else:
        assert rel_l2(c1.float().cpu(), c0.float().cpu()) < 1.5e-2
    with pytest.raises(NotImplementedError):  # outside the envelope: the caller keeps the three launches
        ops.t5_attn_fused_fwd(x[:, :256].contiguous(), gamma[:256], w[:, :256].contiguous(), xn1, r1, p1, c1, l1, cross=cross,
                              k=kv[:, :inner] if cross else None, v=kv[:, inner:] if cross else None, **kw)


@pytest.mark.parametrize("B,H,Lq,Lk,dk,use_bias", [(2, 16, 153, 153, 64, True), (1, 2, 300, 300, 32, True), (2, 3, 200, 90, 64, False)])
def test_t5_attention_long_sequences_streaming_kernels(ops, B, H, Lq, Lk, dk, use_bias):
    """sequences whose Q / K / V / dO images exceed one workgroup's LDS (T5-large encoder: Le = 153 at head dim 64, BASELINE
    configs[4]) run the streaming matrix-core kernels (flash_fwd / flash_bwd_dq / flash_bwd_dkv): forward, d q / d k / d v and
    the position-bias gradient (stored-dS form) against the fp32 reference."""
    dt = torch.bfloat16
    inner = H * dk
    qb, kb, vb = (rnd(B * L_, inner, seed=sd_, scale=0.5).to(dt) for L_, sd_ in ((Lq, 1), (Lk, 2), (Lk, 3)))
    bias = rnd(H, Lq, Lk, seed=4) if use_bias else None
    dctx = rnd(B * Lq, inner, seed=5).to(dt)
    q = qb.float().view(B, Lq, H, dk).transpose(1, 2).clone().requires_grad_(True)
    k = kb.float().view(B, Lk, H, dk).transpose(1, 2).clone().requires_grad_(True)
    v = vb.float().view(B, Lk, H, dk).transpose(1, 2).clone().requires_grad_(True)
    bref = bias.clone().requires_grad_(True) if use_bias else None
    ref = _attn_ref(q, k, v, bref, False)
    ref.backward(dctx.float().view(B, Lq, H, dk).transpose(1, 2))
    ctx = torch.zeros(B * Lq, inner, device="cuda", dtype=dt)
    lse = torch.empty(B, H, Lq, device="cuda")
    kw = dict(B=B, H=H, Lq=Lq, Lk=Lk, dk=dk, bias=dev(bias) if use_bias else None, causal=False)
    qd, kd, vd = dev(qb), dev(kb), dev(vb)
    ops.t5_attn_fwd(qd, kd, vd, ctx, lse, **kw)
    assert rel_l2(ctx.float().cpu(), ref.detach().transpose(1, 2).reshape(B * Lq, inner)) < tol(dt)
    dq, dk_, dv = (torch.zeros(B * L_, inner, device="cuda", dtype=dt) for L_ in (Lq, Lk, Lk))
    dbias = torch.zeros(H, Lq, Lk, device="cuda") if use_bias else None
    ds_ws = torch.empty(B * H * Lq * ((Lk + 31) // 32 * 32), device="cuda", dtype=dt) if use_bias else None
    ops.t5_attn_bwd(qd, kd, vd, ctx, lse, dev(dctx), dq, dk_, dv, dbias=dbias, ds_ws=ds_ws, **kw)
    t = tol(dt) * 2
    assert rel_l2(dq.float().cpu(), q.grad.transpose(1, 2).reshape(B * Lq, inner)) < t
    assert rel_l2(dk_.float().cpu(), k.grad.transpose(1, 2).reshape(B * Lk, inner)) < t
    assert rel_l2(dv.float().cpu(), v.grad.transpose(1, 2).reshape(B * Lk, inner)) < t
    if use_bias:
        assert rel_l2(dbias.cpu(), bref.grad) < t
    # dropout: the mask is a pure function of (seed, tag, b, h, q, key).  Read it out through the kernel itself -- Q = K = 0 gives
    # uniform probabilities 1/Lk, V = one-hot over a chunk of dk keys, so ctx[q, d] = multiplier(q, c0 + d) / Lk -- then check
    # forward AND backward against the reference with exactly that mask.
    sd = seed_word(5)
    pdrop = 0.25
    kwd = dict(B=B, H=H, Lq=Lq, Lk=Lk, dk=dk, drop_p=pdrop, seed=sd, tag=9)
    mask = torch.zeros(B, H, Lq, Lk)
    zq, zk = torch.zeros_like(qd), torch.zeros_like(kd)
    for c0 in range(0, Lk, dk):
        onehot = torch.zeros(B, Lk, H, dk)
        for d in range(min(dk, Lk - c0)):
            onehot[:, c0 + d, :, d] = 1.0
        cc = torch.empty_like(ctx)
        ops.t5_attn_fwd(zq, zk, dev(onehot.reshape(B * Lk, inner).to(dt)), cc, lse, **kwd)
        got = cc.float().cpu().view(B, Lq, H, dk).permute(0, 2, 1, 3) * Lk
        mask[:, :, :, c0:c0 + dk] = got[..., :min(dk, Lk - c0)]
    keep = (mask > 0.5).float()
    assert abs(float(keep.mean()) - (1 - pdrop)) < 0.02 and float((mask * keep).max()) < 1.0 / (1 - pdrop) * 1.02
    q2, k2, v2 = (x.detach().clone().requires_grad_(True) for x in (q, k, v))
    sc = q2 @ k2.transpose(-1, -2) + (bias if use_bias else 0.0)
    ref2 = (torch.softmax(sc, -1) * keep / (1 - pdrop)) @ v2
    ref2.backward(dctx.float().view(B, Lq, H, dk).transpose(1, 2))
    c1 = torch.empty_like(ctx)
    kwd2 = dict(kwd, bias=dev(bias) if use_bias else None)
    ops.t5_attn_fwd(qd, kd, vd, c1, lse, **kwd2)
    assert rel_l2(c1.float().cpu(), ref2.detach().transpose(1, 2).reshape(B * Lq, inner)) < tol(dt)
    ops.t5_attn_bwd(qd, kd, vd, c1, lse, dev(dctx), dq, dk_, dv, **kwd2)
    assert rel_l2(dq.float().cpu(), q2.grad.transpose(1, 2).reshape(B * Lq, inner)) < t
    assert rel_l2(dk_.float().cpu(), k2.grad.transpose(1, 2).reshape(B * Lk, inner)) < t
    assert rel_l2(dv.float().cpu(), v2.grad.transpose(1, 2).reshape(B * Lk, inner)) < t


def test_t5_attention_dropout_fwd_bwd_consistent(ops):
    # with dropout on, backward must regenerate the forward's mask: check d(ctx)/dV numerically via linearity in V
    B, H, L, dk, p = 2, 2, 24, 16, 0.3
    inner = H * dk
    dt = torch.float32
    q, k = dev(rnd(B * L, inner, seed=1)), dev(rnd(B * L, inner, seed=2))
    v1, v2 = dev(rnd(B * L, inner, seed=3)), dev(rnd(B * L, inner, seed=4))
    sd = seed_word(5)
    kw = dict(B=B, H=H, Lq=L, Lk=L, dk=dk, drop_p=p, seed=sd, tag=9)
    lse = torch.empty(B, H, L, device="cuda")
    c1, c2 = torch.empty(B * L, inner, device="cuda"), torch.empty(B * L, inner, device="cuda")
    ops.t5_attn_fwd(q, k, v1, c1, lse, **kw)
    ops.t5_attn_fwd(q, k, v2, c2, lse, **kw)
    # ctx is linear in V for a fixed mask: <dctx, c1 - c2> == <dV, v1 - v2> with dV from backward
    dctx = dev(rnd(B * L, inner, seed=6))
    dq, dk_, dv = (torch.empty(B * L, inner, device="cuda") for _ in range(3))
    ops.t5_attn_bwd(q, k, v1, c1, lse, dctx, dq, dk_, dv, **kw)
    lhs = float((dctx * (c1 - c2)).sum())
    rhs = float((dv * (v1 - v2)).sum())
    assert abs(lhs - rhs) < 1e-3 * max(1.0, abs(lhs))


# ------------------------------------------------------------------------------------------ fp8 forward GEMM (configs[4])
@pytest.mark.parametrize("M,N,K", [(300, 200, 128), (4096, 1536, 512), (77, 64, 1024), (512, 32128, 256), (130, 130, 4096), (4896, 4096, 1024),
                                   (2048, 1024, 4096), (1000, 384, 64), (333, 96, 192), (640, 128, 48), (20000, 512, 128)])
def test_fp8_gemm_matches_emulated_quantisation(ops, M, N, K):
    """klab_quant_fp8_rows + klab_gemm_fp8 (OCP e4m3 operands, per-row scales, fp32 accumulation) against the same quantisation
    emulated in torch: products of e4m3 values are exact in fp32, so only the accumulation order differs."""
    from tests.helpers import fp8_rows
    a = rnd(M, K, seed=1, scale=2.0).to(torch.bfloat16)
    b = rnd(N, K, seed=2, scale=0.05).to(torch.bfloat16)
    a[3] = 0  # an all-zero row: scale 1, no NaN
    qa, sa = fp8_rows(a)
    qb, sb = fp8_rows(b)
    a8, sa_k = ops.quant_fp8_rows(dev(a))
    b8, sb_k = ops.quant_fp8_rows(dev(b))
    assert rel_l2(sa_k.cpu(), sa.view(-1)) < 1e-6 and rel_l2(sb_k.cpu(), sb.view(-1)) < 1e-6
    deq = a8.cpu().view(torch.float8_e4m3fn).float()
    assert float((deq != qa).float().mean()) < 1e-3  # bit-identical bytes but for ties of the 1/scale product
    bias = rnd(N, seed=3)
    ref = (qa @ qb.t()) * sa * sb.view(1, -1)
    for out_dt in (torch.bfloat16, torch.float32):
        c = torch.empty(M, N, device="cuda", dtype=out_dt)
        ops.gemm_fp8(a8, sa_k, b8, sb_k, c)
        assert rel_l2(c.float().cpu(), ref) < (4e-3 if out_dt == torch.bfloat16 else 2e-4)
    c = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
    ops.gemm_fp8(a8, sa_k, b8, sb_k, c, alpha=0.5, bias=dev(bias), act=ops.L.ACT_RELU)
    assert rel_l2(c.float().cpu(), torch.relu(0.5 * ref + bias)) < 4e-3
    res = rnd(M, N, seed=4)
    c32 = torch.empty(M, N, device="cuda")
    ops.gemm_fp8(a8, sa_k, b8, sb_k, c32, residual=dev(res))
    assert rel_l2(c32.cpu(), ref + res) < 2e-4
    # against the unquantised product: the e4m3 round-off itself (2^-4 relative per element, averaged over K)
    assert rel_l2(ref, a.float() @ b.float().t()) < 6e-2
    if K % 128 == 0:  # the block-scaled instruction (csrc/mmf8.hip, v_mfma_scale_f32_16x16x128_f8f6f4 with unit block scales): same numbers
        for out_dt in (torch.bfloat16, torch.float32):
            c = torch.empty(M, N, device="cuda", dtype=out_dt)
            ops.gemm_fp8(a8, sa_k, b8, sb_k, c, name_tag=2)
            assert rel_l2(c.float().cpu(), ref) < (4e-3 if out_dt == torch.bfloat16 else 2e-4)
        c = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
        ops.gemm_fp8(a8, sa_k, b8, sb_k, c, alpha=0.5, bias=dev(bias), act=ops.L.ACT_RELU, name_tag=2)
        assert rel_l2(c.float().cpu(), torch.relu(0.5 * ref + bias)) < 4e-3


@pytest.mark.parametrize("rows,d", [(300, 512), (77, 1024), (4096, 768), (5, 256), (1000, 64)])
def test_rmsnorm_fwd_with_fused_fp8_rows_equals_norm_then_quantise(ops, rows, d):
    """fp8 mode folds the per-token quantisation into the RMS-norm kernel: the e4m3 bytes and scales must be IDENTICAL to
    klab_quant_fp8_rows of the bf16 output the same kernel wrote"""
    x, w = dev(rnd(rows, d, seed=1, scale=3.0)), dev(1 + 0.2 * rnd(d, seed=2))
    x[2] = 0  # an all-zero row
    y0 = torch.empty(rows, d, device="cuda", dtype=torch.bfloat16)
    r0 = torch.empty(rows, device="cuda")
    ops.rmsnorm_fwd(x, w, y=y0, rstd=r0)
    q0, s0 = ops.quant_fp8_rows(y0)
    y1, r1 = torch.empty_like(y0), torch.empty_like(r0)
    q1, s1 = torch.empty(rows, d, device="cuda", dtype=torch.uint8), torch.empty(rows, device="cuda")
    ops.rmsnorm_fwd_q8(x, w, y1, r1, q1, s1)
    # against the plain kernel: the same values up to the last bit of the row statistic (a different summation order)
    assert torch.allclose(r0, r1, rtol=2e-6, atol=0) and rel_l2(y1.float().cpu(), y0.float().cpu()) < 1e-3
    # and exactly what the separate pass makes of the kernel's OWN bf16 output
    q0, s0 = ops.quant_fp8_rows(y1)
    assert torch.equal(s0.view(-1), s1) and torch.equal(q0, q1)


@pytest.mark.parametrize("rows,C", [(1000, 64), (333, 128), (200, 256), (77, 1024), (50, 96)])
def test_layernorm_and_gelu_with_fused_fp8_rows_equal_the_separate_pass(ops, rows, C):
    """fp8 mode, Swin side: LayerNorm (+ shortcut) and GELU emit their rows in e4m3 too; outputs, bytes and scales identical to the
    plain kernel followed by klab_quant_fp8_rows"""
    y, g, b = dev(rnd(rows, C, seed=1).to(torch.bfloat16)), dev(1 + 0.1 * rnd(C, seed=2)), dev(0.1 * rnd(C, seed=3))
    sc = dev(rnd(rows, C, seed=4))
    out0, outt0 = torch.empty(rows, C, device="cuda"), torch.empty(rows, C, device="cuda", dtype=torch.bfloat16)
    m0, r0 = torch.empty(rows, device="cuda"), torch.empty(rows, device="cuda")
    ops.layernorm_fwd(y, g, b, shortcut=sc, out=out0, outt=outt0, mean=m0, rstd=r0)
    q0, s0 = ops.quant_fp8_rows(outt0)
    out1, outt1, m1, r1 = torch.empty_like(out0), torch.empty_like(outt0), torch.empty_like(m0), torch.empty_like(r0)
    q1, s1 = torch.empty(rows, C, device="cuda", dtype=torch.uint8), torch.empty(rows, device="cuda")
    ops.layernorm_fwd_q8(y, g, b, sc, out1, outt1, m1, r1, q1, s1)
    assert torch.equal(out0, out1) and torch.equal(outt0, outt1) and torch.equal(m0, m1) and torch.equal(r0, r1)
    assert torch.equal(s0.view(-1), s1) and torch.equal(q0, q1)
    F4 = 4 * C
    z = dev((2 * rnd(rows, F4, seed=5)).to(torch.bfloat16))
    z[1] = -30.0  # gelu -> 0 everywhere: the all-zero row
    a0 = torch.empty_like(z)
    ops.gelu_fwd(z, a0)
    qa0, sa0 = ops.quant_fp8_rows(a0)
    a1 = torch.empty_like(z)
    qa1, sa1 = torch.empty(rows, F4, device="cuda", dtype=torch.uint8), torch.empty(rows, device="cuda")
    ops.gelu_fwd_q8(z, a1, qa1, sa1)
    assert torch.equal(a0, a1) and torch.equal(sa0.view(-1), sa1) and torch.equal(qa0, qa1)


# ------------------------------------------------------------------------------------------ Swin attention
def _swin_attn_ref(qkv, bias, logit_scale, B, R, w, shift, H, C):
    """HF/swinv2:389-455 + :652-690 on a fused qkv [B*R*R, 3C] (fp32 torch)."""
    hd, n = C // H, w * w
    x = qkv.view(B, R, R, 3 * C)
    if shift > 0:
        x = torch.roll(x, shifts=(-shift, -shift), dims=(1, 2))
    xw = O._window_partition(x, w).view(-1, n, 3 * C)
    q, k, v = (xw[..., i * C:(i + 1) * C].reshape(-1, n, H, hd).transpose(1, 2) for i in range(3))
    s = F.normalize(q, dim=-1) @ F.normalize(k, dim=-1).transpose(-2, -1)
    s = s * torch.clamp(logit_scale.view(H, 1, 1), max=math.log(100.0)).exp() + bias.unsqueeze(0)
    mask = O.swin_shift_mask(R, w, shift, qkv.dtype)
    if mask is not None:
        nW = mask.shape[0]
        s = (s.view(-1, nW, H, n, n) + 2 * mask.unsqueeze(1).unsqueeze(0)).view(-1, H, n, n)
    ctx = (F.softmax(s, -1) @ v).permute(0, 2, 1, 3).reshape(-1, w, w, C)
    ctx = O._window_reverse(ctx, w, R, R)
    if shift > 0:
        ctx = torch.roll(ctx, shifts=(shift, shift), dims=(1, 2))
    return ctx.reshape(B * R * R, C)


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("B,R,w,shift,H,C", [(2, 8, 4, 0, 2, 32), (2, 8, 4, 2, 2, 32), (1, 14, 7, 3, 2, 64), (2, 2, 2, 0, 8, 128),
                                             (2, 14, 7, 0, 1, 32), (2, 28, 7, 3, 3, 96), (3, 8, 4, 2, 2, 64), (2, 7, 7, 0, 4, 128),
                                             # window 8 = 64 tokens, exactly one tile (the reference's default `window8-256`)
                                             (1, 16, 8, 4, 2, 64), (2, 8, 8, 0, 1, 32), (1, 16, 8, 0, 4, 128)])
def test_swin_window_attention_fwd_bwd(ops, dt, B, R, w, shift, H, C):
    n = w * w
    qkv = rnd(B * R * R, 3 * C, seed=1).to(dt)
    bias = 16 * torch.sigmoid(rnd(H, n, n, seed=2))
    ls = torch.log(10 * torch.ones(H)) + 0.3 * rnd(H, seed=3)
    ls[0] = 5.0  # above ln(100): exercises the clamp (zero gradient)
    dctx = rnd(B * R * R, C, seed=4).to(dt)
    qr = qkv.float().clone().requires_grad_(True)
    br, lr = bias.clone().requires_grad_(True), ls.clone().requires_grad_(True)
    ref = _swin_attn_ref(qr, br, lr, B, R, w, shift, H, C)
    ref.backward(dctx.float())
    ctx = torch.empty(B * R * R, C, device="cuda", dtype=dt)
    nW = (R // w) ** 2
    lse = torch.empty(B * nW * H * n, device="cuda")
    kw = dict(B=B, R=R, w=w, shift=shift, H=H, C=C)
    ops.swin_attn_fwd(dev(qkv), ctx, dev(bias), dev(ls), lse, **kw)
    assert rel_l2(ctx.float().cpu(), ref.detach()) < tol(dt)
    dqkv = torch.empty(B * R * R, 3 * C, device="cuda", dtype=dt)
    dbias, dls = torch.zeros(H, n, n, device="cuda"), torch.zeros(H, device="cuda")
    ops.swin_attn_bwd(dev(qkv), ctx, dev(bias), dev(ls), lse, dev(dctx), dqkv, dbias, dls, **kw)
    t = tol(dt) * 4  # cosine logits are scaled by up to 100: bf16 rounding of q-hat / k-hat is amplified accordingly
    assert rel_l2(dqkv.float().cpu(), qr.grad) < t
    assert rel_l2(dbias.cpu(), br.grad) < t
    assert rel_l2(dls.cpu(), lr.grad) < t * 10  # scalar aggregated over all windows with fast-exp probabilities
    assert float(dls[0]) == 0.0
    if dt == torch.bfloat16 and C == H * 32:  # the matrix-core backward ran above: the vector-ALU form must agree with it
        dq2 = torch.empty_like(dqkv)
        db2, dl2 = torch.zeros_like(dbias), torch.zeros_like(dls)
        ops.swin_attn_bwd(dev(qkv), ctx, dev(bias), dev(ls), lse, dev(dctx), dq2, db2, dl2, mfma=False, **kw)
        assert rel_l2(dqkv.float().cpu(), dq2.float().cpu()) < t
        assert rel_l2(dbias.cpu(), db2.cpu()) < t
        assert rel_l2(dls.cpu(), dl2.cpu()) < t * 10
        assert rel_l2(dq2.float().cpu(), qr.grad) < t


def _table_to_dense(btab, index, H, n):
    """bias[h, i, j] = btab[index[i, j], h] (HF/swinv2:418-428 after the 16*sigmoid)"""
    return btab[index.view(-1).long()].view(n, n, H).permute(2, 0, 1).contiguous()


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("B,R,w,shift,H,C", [(1, 12, 12, 0, 2, 64), (1, 24, 12, 6, 2, 64), (1, 24, 24, 0, 1, 32), (2, 48, 24, 12, 1, 32),
                                             (1, 20, 10, 5, 2, 32),
                                             # window 16 = 256 tokens (`swinv2-base-patch4-window16-256`): shifted, and R == w
                                             (1, 32, 16, 8, 2, 64), (2, 16, 16, 0, 1, 32)])
def test_swin_large_window_attention_fwd_bwd(ops, dt, B, R, w, shift, H, C):
    """windows of more than 64 tokens (BASELINE configs[4]: 384 px / window 24 -> n = 576 and 144; HF/swinv2:389-455, 615-618):
    tiled kernels, the position bias looked up in the (2w-1)^2 x H table; checked against the dense-bias reference, in both
    bias forms (table and dense), forward + every gradient incl. d(bias table)."""
    n, ntab = w * w, (2 * w - 1) ** 2
    _coords, index = O.swin_coords_table_and_index(w, 0, torch.float32)
    qkv = rnd(B * R * R, 3 * C, seed=1).to(dt)
    btab = 16 * torch.sigmoid(rnd(ntab, H, seed=2))
    ls = torch.log(10 * torch.ones(H)) + 0.3 * rnd(H, seed=3)
    dctx = rnd(B * R * R, C, seed=4).to(dt)
    qr = qkv.float().clone().requires_grad_(True)
    tr, lr = btab.clone().requires_grad_(True), ls.clone().requires_grad_(True)
    bias_dense = _table_to_dense(tr, index, H, n)
    ref = _swin_attn_ref(qr, bias_dense, lr, B, R, w, shift, H, C)
    ref.backward(dctx.float())
    nW = (R // w) ** 2
    kw = dict(B=B, R=R, w=w, shift=shift, H=H, C=C)
    t = tol(dt) * 4
    forms = ("table", "dense") + (("table-valu",) if dt == torch.bfloat16 and C == H * 32 else ())
    for form in forms:  # bf16 "table" = the matrix-core streaming kernels, "table-valu" = the vector-ALU tiled kernels
        ctx = torch.empty(B * R * R, C, device="cuda", dtype=dt)
        lse = torch.empty(B * nW * H * n, device="cuda")
        dqkv = torch.empty(B * R * R, 3 * C, device="cuda", dtype=dt)
        dls = torch.zeros(H, device="cuda")
        if form.startswith("table"):
            dtab = torch.zeros(ntab, H, device="cuda")
            mf = form == "table"
            ops.swin_attn_fwd(dev(qkv), ctx, None, dev(ls), lse, bias_table=dev(btab), mfma=mf, **kw)
            ops.swin_attn_bwd(dev(qkv), ctx, None, dev(ls), lse, dev(dctx), dqkv, None, dls, bias_table=dev(btab), dbias_table=dtab, mfma=mf, **kw)
            assert rel_l2(dtab.cpu(), tr.grad) < t, form
        else:
            bd = _table_to_dense(btab, index, H, n)
            dbias = torch.zeros(H, n, n, device="cuda")
            ops.swin_attn_fwd(dev(qkv), ctx, dev(bd), dev(ls), lse, **kw)
            ops.swin_attn_bwd(dev(qkv), ctx, dev(bd), dev(ls), lse, dev(dctx), dqkv, dbias, dls, **kw)
            got = torch.zeros(ntab, H).index_add_(0, index.view(-1).long(), dbias.cpu().permute(1, 2, 0).reshape(n * n, H))
            assert rel_l2(got, tr.grad) < t
        assert rel_l2(ctx.float().cpu(), ref.detach()) < tol(dt), form
        assert rel_l2(dqkv.float().cpu(), qr.grad) < t, form
        assert rel_l2(dls.cpu(), lr.grad) < t * 10, form


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("B,R,w,shift,H,C", [(1, 20, 6, 3, 2, 64), (2, 10, 6, 0, 1, 32), (1, 24, 10, 5, 1, 32), (2, 9, 4, 2, 2, 64)])
def test_swin_padded_window_attention_fwd_bwd(ops, dt, B, R, w, shift, H, C):
    """window PADDING (R % w != 0; HF/swinv2:645-650, 675, 688-690): the grid is padded to ceil(R/w)*w with zero input rows that
    still act as keys (k = 0, v = value bias), the shift mask is built on the padded grid, the output is cropped.  Reference = the
    dense-bias window attention on the explicitly padded grid; checked: output, d qkv, d(bias table), d logit_scale, d(value bias)."""
    n, ntab = w * w, (2 * w - 1) ** 2
    Rp = (R + w - 1) // w * w
    _coords, index = O.swin_coords_table_and_index(w, 0, torch.float32)
    qkv = rnd(B * R * R, 3 * C, seed=1).to(dt)
    btab = 16 * torch.sigmoid(rnd(ntab, H, seed=2))
    ls = torch.log(10 * torch.ones(H)) + 0.3 * rnd(H, seed=3)
    vbias = rnd(C, seed=5, scale=0.5)
    dctx = rnd(B * R * R, C, seed=4).to(dt)
    qr = qkv.float().clone().requires_grad_(True)
    tr, lr, vr = btab.clone().requires_grad_(True), ls.clone().requires_grad_(True), vbias.clone().requires_grad_(True)
    xp = F.pad(qr.view(B, R, R, 3 * C), (0, 0, 0, Rp - R, 0, Rp - R))
    padmask = torch.ones(Rp, Rp)
    padmask[:R, :R] = 0
    vb_full = torch.cat([torch.zeros(2 * C), vr if dt == torch.float32 else vr.detach().to(dt).float() + (vr - vr.detach())])  # bf16: the kernel's rounding, straight-through gradient
    xp = xp + padmask[None, :, :, None] * vb_full
    ref = _swin_attn_ref(xp.reshape(B * Rp * Rp, 3 * C), _table_to_dense(tr, index, H, n), lr, B, Rp, w, shift, H, C)
    ref = ref.view(B, Rp, Rp, C)[:, :R, :R].reshape(B * R * R, C)
    ref.backward(dctx.float())
    nW = (Rp // w) ** 2
    kw = dict(B=B, R=R, w=w, shift=shift, H=H, C=C)
    t = tol(dt) * 4
    forms = ("mfma", "valu") if (dt == torch.bfloat16 and C == H * 32) else ("valu",)
    for form in forms:
        mf = form == "mfma"
        ctx = torch.zeros(B * R * R, C, device="cuda", dtype=dt)
        lse = torch.zeros(B * nW * H * n, device="cuda")
        dqkv = torch.zeros(B * R * R, 3 * C, device="cuda", dtype=dt)
        dls, dtab, dvb = torch.zeros(H, device="cuda"), torch.zeros(ntab, H, device="cuda"), torch.zeros(C, device="cuda")
        ops.swin_attn_fwd(dev(qkv), ctx, None, dev(ls), lse, bias_table=dev(btab), v_bias=dev(vbias), mfma=mf, **kw)
        assert rel_l2(ctx.float().cpu(), ref.detach()) < tol(dt), form
        ops.swin_attn_bwd(dev(qkv), ctx, None, dev(ls), lse, dev(dctx), dqkv, None, dls, bias_table=dev(btab), dbias_table=dtab,
                          v_bias=dev(vbias), dv_bias=dvb, mfma=mf, **kw)
        assert rel_l2(dqkv.float().cpu(), qr.grad) < t, form
        assert rel_l2(dtab.cpu(), tr.grad) < t, form
        assert rel_l2(dls.cpu(), lr.grad) < t * 10, form
        assert rel_l2(dvb.cpu(), vr.grad) < t, form


@pytest.mark.parametrize("w,pw,H", [(12, 6, 4), (24, 12, 2), (8, 0, 3)])
def test_swin_cpb_table_fwd_bwd(ops, w, pw, H):
    """table form of the continuous position bias (any window size; HF/swinv2:376-378,418-428,457-492): 16*sigmoid(MLP(coords))
    and the MLP weight gradients from d(bias table), against autograd through the oracle's dense bias."""
    sd = {"continuous_position_bias_mlp.0.weight": rnd(512, 2, seed=1).requires_grad_(True),
          "continuous_position_bias_mlp.0.bias": rnd(512, seed=2).requires_grad_(True),
          "continuous_position_bias_mlp.2.weight": rnd(H, 512, seed=3, scale=0.1).requires_grad_(True)}
    n, ntab = w * w, (2 * w - 1) ** 2
    ref = O.swin_cpb_bias(sd, "", w, pw, H, torch.float32)  # dense [H, n, n]
    G = rnd(H, n, n, seed=4)
    (ref * G).sum().backward()
    coords, index = O.swin_coords_table_and_index(w, pw, torch.float32)
    coords = coords.view(-1, 2).contiguous()
    w0, b0, w2 = (sd[k].detach() for k in ("continuous_position_bias_mlp.0.weight", "continuous_position_bias_mlp.0.bias",
                                           "continuous_position_bias_mlp.2.weight"))
    table = torch.empty(ntab, H, device="cuda")
    btab = torch.empty(ntab, H, device="cuda")
    hidden = torch.empty(ntab, 512, device="cuda")
    ops.swin_cpb_table(dev(coords), dev(w0), dev(b0), dev(w2), table, btab, hidden, heads=H)
    assert rel_l2(_table_to_dense(btab.cpu(), index, H, n), ref.detach()) < 1e-5
    dbtab = torch.zeros(ntab, H).index_add_(0, index.view(-1).long(), G.permute(1, 2, 0).reshape(n * n, H))
    dtable = torch.empty(ntab, H, device="cuda")
    dw0, db0, dw2 = torch.zeros(512, 2, device="cuda"), torch.zeros(512, device="cuda"), torch.zeros(H, 512, device="cuda")
    ops.swin_cpb_table_bwd(dev(dbtab), btab, dev(coords), hidden, dev(w2), dtable, dw0, db0, dw2, heads=H)
    assert rel_l2(dw2.cpu(), sd["continuous_position_bias_mlp.2.weight"].grad) < 2e-5
    assert rel_l2(dw0.cpu(), sd["continuous_position_bias_mlp.0.weight"].grad) < 2e-5
    assert rel_l2(db0.cpu(), sd["continuous_position_bias_mlp.0.bias"].grad) < 2e-5


@pytest.mark.parametrize("w,H", [(4, 2), (7, 4), (2, 8)])
def test_swin_cpb_bias(ops, w, H):
    sd = {"continuous_position_bias_mlp.0.weight": rnd(512, 2, seed=1), "continuous_position_bias_mlp.0.bias": rnd(512, seed=2),
          "continuous_position_bias_mlp.2.weight": rnd(H, 512, seed=3, scale=0.1)}
    ref = O.swin_cpb_bias(sd, "", w, 0, H, torch.float32)
    coords, index = O.swin_coords_table_and_index(w, 0, torch.float32)
    coords = coords.view(-1, 2).contiguous()
    n = w * w
    table = torch.empty(coords.shape[0], H, device="cuda")
    bias = torch.empty(H, n, n, device="cuda")
    ops.swin_cpb_bias(dev(coords), dev(index.to(torch.int32).contiguous().view(-1)), dev(sd["continuous_position_bias_mlp.0.weight"]),
                      dev(sd["continuous_position_bias_mlp.0.bias"]), dev(sd["continuous_position_bias_mlp.2.weight"]), table, bias,
                      n=n, heads=H)
    assert rel_l2(bias.cpu(), ref) < 1e-5


# ------------------------------------------------------------------------------------------ glue
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("rows,V", [(21, 384), (64, 32128), (5, 512), (9, 16384), (7, 16392), (3, 32768), (3, 40000)])
def test_cross_entropy(ops, dt, rows, V):
    logits = rnd(rows, V, seed=1, scale=3.0).to(dt)
    labels = torch.randint(0, V, (rows,), generator=torch.Generator().manual_seed(3))
    labels[1] = -100
    labels[rows - 1] = 0
    lr = logits.float().clone().requires_grad_(True)
    ref = F.cross_entropy(lr, labels, ignore_index=-100)
    ref.backward()
    lg = dev(logits).clone()
    inv_n, loss_row, loss = torch.empty(1, device="cuda"), torch.empty(rows, device="cuda"), torch.empty(1, device="cuda")
    ops.ce_fwd(lg, dev(labels), inv_n, loss_row, loss, write_grad=True)
    assert abs(float(loss) - float(ref)) < 1e-5 * abs(float(ref)) + 1e-6
    assert rel_l2(lg.float().cpu(), lr.grad) < (2e-5 if dt == torch.float32 else 6e-3)
    assert float(lg[1].abs().max()) == 0.0
    lg2 = dev(logits).clone()
    ops.ce_fwd(lg2, dev(labels), inv_n, loss_row, loss, write_grad=False)
    assert torch.equal(lg2, dev(logits))


def test_embedding_shift_right_and_scatter(ops):
    V, d, B, L = 50, 32, 3, 6
    table = rnd(V, d, seed=1)
    labels = torch.randint(1, V, (B, L), generator=torch.Generator().manual_seed(2))
    labels[0, 2] = -100
    cfg = O.T5Cfg()
    ids = O.t5_shift_right(labels, cfg)
    out = torch.empty(B * L, d, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    ops.embed_fwd(dev(labels), dev(table), out, shift_right=True, L_seq=L, start_id=0, pad_id=0, err=err)
    assert torch.equal(out.cpu(), table[ids.view(-1)])
    assert int(err) == 0
    dh = rnd(B * L, d, seed=3)
    dtab = torch.zeros(V, d, device="cuda")
    ops.embed_bwd(dev(labels), dev(dh), dtab, shift_right=True, L_seq=L)
    ref = torch.zeros(V, d).index_add_(0, ids.view(-1), dh)
    assert rel_l2(dtab.cpu(), ref) < 1e-6
    # plain gather + out-of-range id flag
    bad = torch.tensor([1, 2, V + 3], dtype=torch.long)
    o2 = torch.empty(3, d, device="cuda")
    ops.embed_fwd(dev(bad), dev(table), o2, err=err)
    assert int(err) == 1


def test_relative_bias_gather_scatter(ops):
    H, Lq, Lk = 4, 9, 13
    cfg = O.T5Cfg(num_heads=H)
    table = rnd(32, H, seed=1)
    ctx = torch.arange(Lq)[:, None]
    mem = torch.arange(Lk)[None, :]
    bucket = O.t5_relative_position_bucket(mem - ctx, True, 32, 128).to(torch.int32).contiguous()
    bias = torch.empty(H, Lq, Lk, device="cuda")
    ops.relbias_fwd(dev(table), dev(bucket), bias)
    ref = O.t5_position_bias(table, Lq, Lk, True, cfg)[0]
    assert torch.equal(bias.cpu(), ref)
    db = rnd(H, Lq, Lk, seed=2)
    dtab = torch.zeros(32, H, device="cuda")
    ops.relbias_bwd(dev(db), dev(bucket), dtab)
    tr = table.clone().requires_grad_(True)
    O.t5_position_bias(tr, Lq, Lk, True, cfg)[0].backward(db)
    assert rel_l2(dtab.cpu(), tr.grad) < 1e-5


@pytest.mark.parametrize("dt", DT)
def test_patch_embed_as_gemm_and_merge(ops, dt):
    B, Cin, Himg, P, Cout = 2, 3, 16, 4, 16
    pix, wconv, bconv = rnd(B, Cin, Himg, Himg, seed=1), rnd(Cout, Cin, P, P, seed=2), rnd(Cout, seed=3)
    R = Himg // P
    cols = torch.empty(B * R * R, Cin * P * P, device="cuda", dtype=dt)
    ops.im2col_patch(dev(pix), cols, P)
    out = torch.empty(B * R * R, Cout, device="cuda")
    ops.gemm(cols, dev(wconv.view(Cout, -1).contiguous(), dt), out, M=B * R * R, N=Cout, K=Cin * P * P, bias=dev(bconv))
    ref = F.conv2d(pix, wconv, bconv, stride=P).flatten(2).transpose(1, 2).reshape(B * R * R, Cout)
    assert rel_l2(out.cpu(), ref) < tol(dt)
    # patch merging gather order (HF/swinv2:342-351) and its scatter
    C = 8
    x = rnd(B, R, R, C, seed=4)
    f = torch.cat([x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]], -1).reshape(-1, 4 * C)
    mg = torch.empty(B * (R // 2) ** 2, 4 * C, device="cuda", dtype=dt)
    ops.merge_gather(dev(x), mg, B=B, R=R, C=C)
    assert rel_l2(mg.float().cpu(), f) < (1e-7 if dt == torch.float32 else 4e-3)
    back = torch.empty(B, R, R, C, device="cuda")
    ops.merge_scatter(dev(f.contiguous()), back, B=B, R=R, C=C)
    assert torch.equal(back.cpu(), x)


@pytest.mark.parametrize("dt", DT)
def test_colsum_and_convert(ops, dt):
    M, N = 300, 72
    dy = rnd(M, N, seed=1).to(dt)
    out = torch.zeros(N, device="cuda")
    ops.colsum(dev(dy), out)
    assert rel_l2(out.cpu(), dy.float().sum(0)) < 1e-5
    big = dev(rnd(5003, 288, seed=3).to(dt))  # column slices of a wider matrix (the v-bias gradient reads dqkv[:, 2C:])
    for c0, nc in ((0, 96), (192, 96), (8, 200)):
        o2 = torch.zeros(nc, device="cuda")
        ops.colsum(big[:, c0:c0 + nc], o2)
        assert rel_l2(o2.cpu(), big[:, c0:c0 + nc].float().sum(0).cpu()) < 1e-5
    x = rnd(64, 16, seed=2)
    y = torch.empty(64, 16, device="cuda", dtype=dt)
    ops.convert(dev(x), y, 0.5)
    assert rel_l2(y.float().cpu(), 0.5 * x) < (1e-7 if dt == torch.float32 else 4e-3)


@pytest.mark.gpu
@pytest.mark.parametrize("M,Cc", [(300, 64), (128, 64), (1000, 128), (77, 128)])
def test_swin_mlp_fused_matches_torch(ops, M, Cc):
    """Fused frozen-tower MLP half == fc1 -> erf-GELU -> fc2 -> LayerNorm -> + shortcut in fp32 torch (HF/swinv2:539-563,697-702)
    on the same bf16-rounded operands; tolerance = bf16 rounding of the hidden activations."""
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(M, Cc, generator=g)).to(torch.bfloat16)
    sc = torch.randn(M, Cc, generator=g)
    w1 = (torch.randn(4 * Cc, Cc, generator=g) / Cc ** 0.5).to(torch.bfloat16)
    w2 = (torch.randn(Cc, 4 * Cc, generator=g) / (4 * Cc) ** 0.5).to(torch.bfloat16)
    b1, b2 = torch.randn(4 * Cc, generator=g) * 0.1, torch.randn(Cc, generator=g) * 0.1
    gm, bt = torch.rand(Cc, generator=g) + 0.5, torch.randn(Cc, generator=g) * 0.1
    h = F.gelu(x.float() @ w1.float().t() + b1).to(torch.bfloat16).float()
    y = h @ w2.float().t() + b2
    ref = sc + F.layer_norm(y, (Cc,), gm, bt, 1e-5)
    gout = torch.full((M + 8, Cc), 7.0, device="cuda")  # 8 guard rows: nothing past row M may be written (ragged M: 300, 77)
    goutt = torch.full((M + 8, Cc), 7.0, device="cuda", dtype=torch.bfloat16)
    out, outt = gout[:M], goutt[:M]
    ops.swin_mlp_fused(dev(x), dev(sc), dev(w1), dev(b1), dev(w2), dev(b2), dev(gm), dev(bt), out, outt, eps=1e-5)
    assert rel_l2(out.cpu(), ref) < 4e-3
    assert rel_l2(outt.float().cpu(), ref) < 8e-3
    assert bool((gout[M:] == 7.0).all()) and bool((goutt[M:] == 7.0).all())
    if Cc == 64:
        with pytest.raises(NotImplementedError):
            bad = torch.zeros(8, 256, device="cuda", dtype=torch.bfloat16)
            ops.swin_mlp_fused(bad, torch.zeros(8, 256, device="cuda"), torch.zeros(1024, 256, device="cuda", dtype=torch.bfloat16),
                               torch.zeros(1024, device="cuda"), torch.zeros(256, 1024, device="cuda", dtype=torch.bfloat16),
                               torch.zeros(256, device="cuda"), torch.ones(256, device="cuda"), torch.zeros(256, device="cuda"),
                               torch.empty(8, 256, device="cuda"))


@pytest.mark.gpu
@pytest.mark.parametrize("M,Cc", [(300, 64), (1000, 128)])
def test_swin_proj_ln_fused_matches_torch(ops, M, Cc):
    """Fused frozen-tower attention-output half == Linear -> LayerNorm -> + shortcut in fp32 torch (HF/swinv2:496-506, 697-700)."""
    g = torch.Generator().manual_seed(6)
    x = torch.randn(M, Cc, generator=g).to(torch.bfloat16)
    sc = torch.randn(M, Cc, generator=g)
    w = (torch.randn(Cc, Cc, generator=g) / Cc ** 0.5).to(torch.bfloat16)
    b = torch.randn(Cc, generator=g) * 0.1
    gm, bt = torch.rand(Cc, generator=g) + 0.5, torch.randn(Cc, generator=g) * 0.1
    ref = sc + F.layer_norm(x.float() @ w.float().t() + b, (Cc,), gm, bt, 1e-5)
    gout = torch.full((M + 8, Cc), 7.0, device="cuda")  # 8 guard rows: nothing past row M may be written
    goutt = torch.full((M + 8, Cc), 7.0, device="cuda", dtype=torch.bfloat16)
    out, outt = gout[:M], goutt[:M]
    ops.swin_proj_ln_fused(dev(x), dev(sc), dev(w), dev(b), dev(gm), dev(bt), out, outt, eps=1e-5)
    assert rel_l2(out.cpu(), ref) < 1e-3
    assert rel_l2(outt.float().cpu(), ref) < 6e-3
    assert bool((gout[M:] == 7.0).all()) and bool((goutt[M:] == 7.0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("R,Cc,Hh,shift,w", [(14, 64, 2, 0, 7), (14, 64, 2, 3, 7), (14, 128, 4, 3, 7), (7, 128, 4, 0, 7), (14, 256, 8, 3, 7),
                                             (14, 256, 8, 0, 7), (16, 64, 2, 4, 8), (8, 128, 4, 0, 8), (16, 256, 8, 4, 8)])  # window 8: n = 64
def test_swin_qkv_attn_fused_matches_two_kernel_path(ops, R, Cc, Hh, shift, w):
    """Frozen-tower fusion == klab_gemm (q|k|v projection) followed by klab_swin_attn_fwd on the same inputs (which the oracle
    pins, test_swin_attn_*): the only difference is that q|k|v are not rounded to bf16 before the cosine normalisation."""
    B = 3
    n = w * w
    g = torch.Generator().manual_seed(9)
    M = B * R * R
    x = torch.randn(M, Cc, generator=g).to(torch.bfloat16)
    wq = (torch.randn(3 * Cc, Cc, generator=g) / Cc ** 0.5).to(torch.bfloat16)
    bq = torch.randn(3 * Cc, generator=g) * 0.2
    bq[Cc:2 * Cc] = 0
    bias = torch.randn(Hh, n, n, generator=g)
    ls = torch.full((Hh,), 2.0)
    qkv = torch.empty(M, 3 * Cc, device="cuda", dtype=torch.bfloat16)
    ops.gemm(dev(x), dev(wq), qkv, M=M, N=3 * Cc, K=Cc, bias=dev(bq))
    ref = torch.empty(M, Cc, device="cuda", dtype=torch.bfloat16)
    ops.swin_attn_fwd(qkv, ref, dev(bias), dev(ls), None, B=B, R=R, w=w, shift=shift, H=Hh, C=Cc)
    out = torch.empty(M, Cc, device="cuda", dtype=torch.bfloat16)
    ops.swin_qkv_attn_fused(dev(x), dev(wq), dev(bq), out, dev(bias), dev(ls), B=B, R=R, w=w, shift=shift, H=Hh, C=Cc)
    assert rel_l2(out.float().cpu(), ref.float().cpu()) < 1.5e-2


@pytest.mark.parametrize("B,HW,Cc", [(3, 224, 64), (2, 56, 96), (1, 384, 128), (5, 28, 64)])
def test_swin_patch_embed_fused_matches_torch(ops, B, HW, Cc):
    """Frozen-tower patch embedding in one launch == Conv2d(3 -> C, k 4, s 4) -> LayerNorm in fp32 torch (HF/swinv2:234-259, 281,
    293-302) on bf16-rounded weights / pixels (the operands the matrix cores see), the convolution output rounded to bf16 before the
    norm as the three-launch path stores it."""
    g = torch.Generator().manual_seed(3)
    pix = torch.randn(B, 3, HW, HW, generator=g)
    w = torch.randn(Cc, 3, 4, 4, generator=g) * 0.1
    bias, gamma, beta = torch.randn(Cc, generator=g) * 0.1, 1 + 0.2 * torch.randn(Cc, generator=g), 0.1 * torch.randn(Cc, generator=g)
    wp = torch.zeros(Cc, 64, dtype=torch.bfloat16)
    wp[:, :48] = w.reshape(Cc, 48).to(torch.bfloat16)
    conv = F.conv2d(pix.to(torch.bfloat16).float(), w.to(torch.bfloat16).float(), bias, stride=4)  # [B, C, R, R]
    y = conv.flatten(2).transpose(1, 2).reshape(-1, Cc).to(torch.bfloat16).float()
    ref = F.layer_norm(y, (Cc,), gamma, beta, 1e-5)
    R = HW // 4
    M = B * R * R
    gout = torch.full((M + 8, Cc), 7.0, device="cuda")  # 8 guard rows: nothing past row M may be written
    goutt = torch.full((M + 8, Cc), 7.0, device="cuda", dtype=torch.bfloat16)
    out, outt = gout[:M], goutt[:M]
    ops.swin_patch_embed_fused(dev(pix), dev(wp), dev(bias), dev(gamma), dev(beta), out, outt)
    assert bool((gout[M:] == 7.0).all()) and bool((goutt[M:] == 7.0).all())
    assert rel_l2(out.cpu(), ref) < 4e-3, rel_l2(out.cpu(), ref)  # (a bf16 rounding flip of the conv output moves a normalised value by ~0.4 %)
    assert rel_l2(outt.float().cpu(), ref) < 6e-3
    with pytest.raises(NotImplementedError):
        ops.swin_patch_embed_fused(dev(pix), dev(wp), dev(bias), dev(gamma), dev(beta), out, outt, patch=2)


@pytest.mark.parametrize("M,K", [(12544, 256), (12544, 1024), (200, 128), (64, 256), (777, 512), (100, 160), (31, 1024)])
def test_swin_linear_ln_fused_matches_torch(ops, M, K):
    """Frozen-tower wide stage: shortcut + LayerNorm(x W^T + b) in one launch == fp32 torch on the bf16-rounded operands, the Linear's
    output rounded to bf16 before the norm as the two-launch path stores it (HF/swinv2:496-506 / 555-563 + 697-702).  Ragged row
    counts (the last workgroup's rows past M) and both call sites' K (C and 4C at C = 256) are covered."""
    Cc = 256
    g = torch.Generator().manual_seed(11)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16)
    w = (torch.randn(Cc, K, generator=g) / math.sqrt(K)).to(torch.bfloat16)
    bias, gamma, beta = torch.randn(Cc, generator=g) * 0.1, 1 + 0.2 * torch.randn(Cc, generator=g), 0.1 * torch.randn(Cc, generator=g)
    shortcut = torch.randn(M, Cc, generator=g)
    y = (x.float() @ w.float().T + bias).to(torch.bfloat16).float()
    ref = shortcut + F.layer_norm(y, (Cc,), gamma, beta, 1e-5)
    out = torch.full((M + 8, Cc), 7.0, device="cuda")  # 8 guard rows: nothing past row M may be written
    outt = torch.full((M + 8, Cc), 7.0, device="cuda", dtype=torch.bfloat16)
    ops.swin_linear_ln_fused(dev(x), dev(shortcut), dev(w), dev(bias), dev(gamma), dev(beta), out[:M], outt[:M])
    assert rel_l2(out[:M].cpu(), ref) < 3e-3, rel_l2(out[:M].cpu(), ref)  # (bf16 rounding flips of the Linear's output)
    assert rel_l2(outt[:M].float().cpu(), ref) < 5e-3
    assert torch.equal(outt[:M].cpu(), out[:M].to(torch.bfloat16).cpu())
    assert bool((out[M:] == 7.0).all()) and bool((outt[M:] == 7.0).all())
    with pytest.raises(NotImplementedError):  # widths other than 256 stay on the two-launch path
        ops.swin_linear_ln_fused(dev(x), dev(shortcut[:, :128].contiguous()), dev(w[:128].contiguous()), dev(bias[:128]), dev(gamma[:128]),
                                 dev(beta[:128]), out[:M, :128].contiguous(), None)


def test_error_paths_of_the_entry_points_added_in_round_two(ops):
    """bad arguments and unsupported shapes come back as KLAB_ERR_* (ValueError / NotImplementedError), never as a launch"""
    import ctypes as C
    from klab_multimodalmodel_amd import _lib as L
    lib = L.load()
    x = torch.zeros(4, 2048, device="cuda")
    w = torch.ones(2048, device="cuda")
    y = torch.zeros(4, 2048, device="cuda", dtype=torch.bfloat16)
    y8 = torch.zeros(4, 2048, device="cuda", dtype=torch.uint8)
    sc = torch.zeros(4, device="cuda")
    with pytest.raises(NotImplementedError):  # rows wider than the register-resident form
        ops.rmsnorm_fwd_q8(x, w, y, None, y8, sc)
    with pytest.raises(ValueError):
        L.check(lib.klab_rmsnorm_fwd_q8(x.data_ptr(), w.data_ptr(), None, None, y8.data_ptr(), sc.data_ptr(), 4, 2048, 1e-6, 0.0, None, 0, None), "q8")
    z = torch.zeros(2, 8192, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(NotImplementedError):
        ops.gelu_fwd_q8(z, torch.empty_like(z), torch.zeros(2, 8192, device="cuda", dtype=torch.uint8), torch.zeros(2, device="cuda"))
    with pytest.raises(ValueError):  # the bias-gradient form needs the row result it sums
        L.check(lib.klab_layernorm_bwd_bias(x.data_ptr(), y.data_ptr(), L.BF16, w.data_ptr(), sc.data_ptr(), sc.data_ptr(), None, None, None,
                                            w.data_ptr(), 4, 2048, 0, 0, 0, 0.0, None, 0, None), "ln")
    # JPEG device half: an item the header marked unsupported, and a workspace that is too small
    items = (L.JpegItem * 1)()
    items[0].info.width = items[0].info.height = 8
    items[0].info.ncomp = 1
    items[0].info.hmax = items[0].info.vmax = 1
    items[0].info.hs[0] = items[0].info.vs[0] = 1
    items[0].info.bw[0] = items[0].info.bh[0] = 1
    items[0].info.coef_blocks = 1
    buf = torch.zeros(1 << 16, device="cuda", dtype=torch.uint8)
    args = (buf.data_ptr(), buf.data_ptr(), C.cast(items, C.c_void_p), buf.data_ptr(), 1, buf.data_ptr(), buf.data_ptr())
    with pytest.raises(NotImplementedError):
        L.check(lib.klab_jpeg_decode_device(*args, 1 << 16, None), "jpeg")
    items[0].info.supported = 1
    with pytest.raises(ValueError):
        L.check(lib.klab_jpeg_decode_device(*args, 16, None), "jpeg")
    assert lib.klab_jpeg_decode_ws_bytes(C.cast(items, C.c_void_p), 1) >= 64
    torch.cuda.synchronize()


@pytest.mark.parametrize("M,N,K,pad", [(384, 256, 128, 0), (300, 264, 96, 0), (256, 128, 64, 4), (1000, 512, 256, 0)])
def test_gemm_dgelu_aux_epilogue(ops, M, N, K, pad):
    """dZ = (dY @ W) * gelu'(Z) (the trainable Swin MLP backward, HF/swinv2:539-563 under autograd): the copy-out form (whole
    16-byte pieces of Z) and, with a row pitch of Z that is not a multiple of 8 elements, the in-register form"""
    dt = torch.bfloat16
    dy, w = rnd(M, K, seed=1).to(dt), rnd(K, N, seed=2, scale=0.2).to(dt)
    zfull = (2 * rnd(M, N + pad, seed=3)).to(dt)
    z = zfull[:, :N]
    ref = (dy.float() @ w.float()) * (0.5 * (1 + torch.erf(z.float() / 2 ** 0.5)) + z.float() * torch.exp(-0.5 * z.float() ** 2) / (2 * torch.pi) ** 0.5)
    zd = dev(zfull)[:, :N]
    c = torch.empty(M, N, device="cuda", dtype=dt)
    ops.gemm(dev(dy), dev(w), c, M=M, N=N, K=K, a_kmajor=True, b_kmajor=False, aux=zd, aux_mode=ops.L.AUX_DGELU)
    assert rel_l2(c.float().cpu(), ref) < 8e-3


@pytest.mark.parametrize("M,N,K,bk", [(4896, 1024, 1024, True), (4900, 1000, 1056, True), (4896, 1024, 2048, False), (2048, 4096, 1024, True)])
def test_gemm_eight_wave_256x128_tiles(ops, M, N, K, bk):
    """the products the dispatcher gives to gemm_glds_w8_kernel (K >= 1024, more than 256 tiles of 128 x 128, at most 256 of
    256 x 128): K-major and m-major B, ragged M / N edges, bf16 and f32 outputs, residual copy-out, bias + ReLU"""
    dt = torch.bfloat16
    A = rnd(M, K, seed=1).to(dt)
    B = (rnd(N, K, seed=2, scale=0.05) if bk else rnd(K, N, seed=2, scale=0.05)).to(dt)
    ref = A.float() @ (B.float().t() if bk else B.float())
    for out_dt in (dt, torch.float32):
        c = torch.empty(M, N, device="cuda", dtype=out_dt)
        ops.gemm(dev(A), dev(B), c, M=M, N=N, K=K, b_kmajor=bk)
        assert rel_l2(c.float().cpu(), ref) < (4e-3 if out_dt == dt else 1e-5)
    res, bias = rnd(M, N, seed=3), rnd(N, seed=4)
    c = torch.empty(M, N, device="cuda")
    ops.gemm(dev(A), dev(B), c, M=M, N=N, K=K, b_kmajor=bk, residual=dev(res))
    assert rel_l2(c.cpu(), ref + res) < 1e-5
    c = torch.empty(M, N, device="cuda", dtype=dt)
    ops.gemm(dev(A), dev(B), c, M=M, N=N, K=K, b_kmajor=bk, bias=dev(bias), act=ops.L.ACT_RELU)
    assert rel_l2(c.float().cpu(), torch.relu(ref + bias)) < 4e-3


# k-extent classes of the LDS-DMA ring's main loop (csrc/gemm_glds_loop.h; S = 4 stages).  nt = k-tiles per workgroup.
_RING_BF16_K = [32, 64, 96, 128, 160, 224, 256, 288, 352, 384, 416]  # BK = 32: nt = 1, 2, 3, 4, 5, 7, 8, 9, 11, 12, 13
_RING_CASES = ([("bf16", True, True, k) for k in _RING_BF16_K]
               + [("bf16", True, False, 224), ("bf16", False, False, 256), ("bf16", False, True, 352)]
               + [("w8", True, True, k) for k in (1088, 1120)]        # with 1024 / 1056 / 2048 of the test above: every nt mod 4
               + [("fp8", True, True, k) for k in (64, 128, 256, 320, 512, 576, 768)])  # BK = 64: nt = 1, 2, 4, 5, 8, 9, 12


@pytest.mark.parametrize("kind,ak,bk,K", _RING_CASES)
def test_gemm_glds_ring_k_extent_classes(ops, kind, ak, bk, K):
    """every way through the ring loop: a prologue shorter than the ring (nt < 4), the four-left drain straight after the prologue
    (nt = 4) and after one steady round (nt = 8, 12), every exit of the general tail after no (nt = 5, 7) and one steady round
    (nt = 9, 11, 13).  bf16: M = N = 64 is one workgroup of gemm_glds_kernel<64, 64> (reference and tolerance of
    test_gemm_nt_epilogues / test_gemm_nn_tn_layouts); w8: gemm_glds_w8_kernel, which has no drain (those of
    test_gemm_eight_wave_256x128_tiles); fp8: gemm_glds_fp8_kernel<64, 64> at the smallest M, N its dispatch accepts (those of
    test_fp8_gemm_matches_emulated_quantisation)."""
    dt = torch.bfloat16
    if kind == "fp8":
        from tests.helpers import fp8_rows
        M = N = 16
        a = rnd(M, K, seed=1, scale=2.0).to(dt)
        b = rnd(N, K, seed=2, scale=0.05).to(dt)
        qa, sa = fp8_rows(a)
        qb, sb = fp8_rows(b)
        a8, sa_k = ops.quant_fp8_rows(dev(a))
        b8, sb_k = ops.quant_fp8_rows(dev(b))
        ref = (qa @ qb.t()) * sa * sb.view(1, -1)
        for out_dt in (dt, torch.float32):
            c = torch.empty(M, N, device="cuda", dtype=out_dt)
            ops.gemm_fp8(a8, sa_k, b8, sb_k, c)
            assert rel_l2(c.float().cpu(), ref) < (4e-3 if out_dt == dt else 2e-4)
        return
    if kind == "w8":
        M, N = 4896, 1024
        A = rnd(M, K, seed=1).to(dt)
        B = rnd(N, K, seed=2, scale=0.05).to(dt)
        ref = A.float() @ B.float().t()
        for out_dt in (dt, torch.float32):
            c = torch.empty(M, N, device="cuda", dtype=out_dt)
            ops.gemm(dev(A), dev(B), c, M=M, N=N, K=K)
            assert rel_l2(c.float().cpu(), ref) < (4e-3 if out_dt == dt else 1e-5)
        return
    M = N = 64
    A = rnd(*((M, K) if ak else (K, M)), seed=1).to(dt)
    B = rnd(*((N, K) if bk else (K, N)), seed=2).to(dt)
    ref = (A.float() if ak else A.float().t()) @ (B.float().t() if bk else B.float())
    Cf = torch.empty(M, N, device="cuda")
    ops.gemm(dev(A), dev(B), Cf, M=M, N=N, K=K, a_kmajor=ak, b_kmajor=bk)
    assert rel_l2(Cf.cpu(), ref) < tol(dt)
    Ct = torch.empty(M, N, device="cuda", dtype=dt)
    ops.gemm(dev(A), dev(B), Ct, M=M, N=N, K=K, a_kmajor=ak, b_kmajor=bk)
    assert rel_l2(Ct.float().cpu(), ref) < tol(dt) * 1.5
