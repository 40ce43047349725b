"""Exact and per-element reference tests of the frozen Swin tower's Linear (+ GELU + Linear) + LayerNorm (+ residual) kernels:
klab_swin_proj_ln_fused, klab_swin_mlp_fused (csrc/swin_mlp.hip), klab_swin_linear_ln_fused (csrc/swin_lin_ln.hip) and
klab_swin_patch_embed_fused (csrc/swin_embed.hip).  References, fixtures and bounds: tests/frozen_tower_ref.py.

rule of the kernel                                                   -> smallest shape that can break it
  mlp, proj: a workgroup owns 128 rows, a wave 32 (two tiles of 16)  -> M = 1, 33 (wave 1 ragged, waves 2-3 wholly past the edge: "rows
                                                                        past the edge are a copy of the last row and never stored"),
                                                                        128, 129 (second workgroup of one row), 300
  mlp: weights stream in chunks of 64 hidden units, S slots deep      -> C = 64 (ring of 3, 4 chunks), C = 128 (ring of 2, 8 chunks);
                                                                        C = 256 is refused and touches nothing
  mlp: GELU by polynomial, hidden row stored as bf16                 -> the sweep case: M = 129, one hidden unit per channel, every
                                                                        multiple of 1/64 in [-6, 6) as a pre-activation
  proj: the chunk's 64 "hidden units" are output channels             -> C = 64 (one chunk: the prologue issues the only one), C = 128 (two)
  linear_ln: 4-slot ring of 32-deep k-tiles, three in flight          -> K = 128 (4 tiles, one lap), 160 (5: no multiple of the ring)
             32-row workgroups below K = 512, 64-row from there       -> K = 480 (the largest at 32 rows), 512, 544, 1024
             rows past the edge are a copy of the last row            -> M = 1, 31, 33, 100 at 32 rows; M = 63, 65, 130 at 64 rows
             envelope: C = 256, K % 32 == 0, K >= 128                 -> C = 128, K = 96, K = 144 are refused
  patch_embed: a wave owns 16 patches, a workgroup 64                 -> (B, HW) = (3, 12): M = 27, a tile spans image rows and images;
                                                                        (1, 32): M = 64, exactly one workgroup; (5, 28): M = 245, wave 3
                                                                        of the last workgroup ragged; (1, 4): M = 1
               C in {64, 96, 128}; weight pitch >= 64, columns 48-63 zero -> every C at pitch 64 and 72; patch = 2 and C = 256 refused
rstd chain (longest f32 addition chain of the variance sum): proj, mlp, patch_embed C / 4 + 2; linear_ln C / 4 + 2 + 3 = 69.

Level 1 (integer fixtures): the kernel's rstd is read at the probe element of every row and held against fp64 within
(chain + 8) 2^-24 rstd; every element of out must equal f32(f32(f32(f32(d rho) gamma) + beta) + shortcut) of that rho, outt its
bf16 rounding, bit for bit.  Level 2 (randn): every element against fp64 within the derived bound, factor 1.
Every output lies between guard bands and starts as NaN; each kernel also runs with outt = None; the inputs are compared with
their copies afterwards."""
import pytest
import torch

from tests import frozen_tower_ref as T
from tests.rowops_ref import U24, Guarded, assert_equal, assert_within

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module")
def ops():
    from klab_multimodalmodel_amd import ops as K
    return K


def cu(t, dtype=F32):
    return t.to(dtype).cuda().contiguous()


def padded_weight(W, pitch):
    """[C, 48] -> the bf16 [C, 64] view of a [C, pitch] buffer: columns 48 .. 63 zero, whatever lies behind them is not the kernel's"""
    buf = torch.full((W.shape[0], pitch), 5.0, dtype=BF16)
    buf[:, :64] = 0.0
    buf[:, :48] = W.to(BF16)
    return buf.cuda()[:, :64]


def device_operands(fx, pitch=64):
    k = fx["kernel"]
    t = dict(gamma=cu(fx["gamma"]), beta=cu(fx["beta"]), b=cu(fx["b"]))
    if k == "patch_embed":
        t.update(pix=cu(fx["pix"]), W=padded_weight(fx["W"], pitch))
    else:
        t.update(x=cu(fx["x"], BF16), sc=cu(fx["sc"]), W=cu(fx["W"], BF16))
    if k == "mlp":
        t.update(W1=cu(fx["W1"], BF16), b1=cu(fx["b1"]))
    return t


def launch(ops, kernel, t, out, outt):
    if kernel == "proj":
        ops.swin_proj_ln_fused(t["x"], t["sc"], t["W"], t["b"], t["gamma"], t["beta"], out, outt, eps=T.EPS)
    elif kernel == "mlp":
        ops.swin_mlp_fused(t["x"], t["sc"], t["W1"], t["b1"], t["W"], t["b"], t["gamma"], t["beta"], out, outt, eps=T.EPS)
    elif kernel == "linear_ln":
        ops.swin_linear_ln_fused(t["x"], t["sc"], t["W"], t["b"], t["gamma"], t["beta"], out, outt, eps=T.EPS)
    else:
        ops.swin_patch_embed_fused(t["pix"], t["W"], t["b"], t["gamma"], t["beta"], out, outt, eps=T.EPS)


def run(ops, kernel, t, M, C, tag):
    """both calls (with and without outt) between guard bands; the inputs must come back as they went in"""
    before = {k: v.clone() for k, v in t.items()}
    out, outt, alone = Guarded((M, C), F32), Guarded((M, C), BF16), Guarded((M, C), F32)
    launch(ops, kernel, t, out.t, outt.t)
    launch(ops, kernel, t, alone.t, None)
    torch.cuda.synchronize()
    for k, v in t.items():
        assert_equal(f"{kernel} input {k} after the call", v, before[k], tag)
    o, ot, oa = out.check(f"{kernel} out{tag}"), outt.check(f"{kernel} outt{tag}"), alone.check(f"{kernel} out (outt = None){tag}")
    for name, v in ((" out", o), (" outt", ot), (" out (outt = None)", oa)):
        nan = torch.isnan(v.float())
        assert not bool(nan.any()), f"{kernel}{name}{tag}: {int(nan.sum())} elements never written, first at {tuple(nan.nonzero()[0].tolist())}"
    assert_equal(f"{kernel} out (outt = None) against out", oa, o, tag)
    return o, ot


def check_exact(ops, fx, M, tag, pitch=64):
    kernel, C = fx["kernel"], fx["C"]
    o, ot = run(ops, kernel, device_operands(fx, pitch), M, C, tag)
    rho_k = o[torch.arange(M), fx["probe"]]
    n = T.chain(kernel, C)
    assert_within(f"{kernel} rstd (read at the probe, chain {n})", rho_k, fx["rho"], (n + 8) * U24 * fx["rho"], tag)
    want = T.expected_out(fx, rho_k)
    assert_equal(f"{kernel} out", o, want, tag)
    assert_equal(f"{kernel} outt", ot, want.to(BF16), tag)


def check_randn(ops, fx, M, tag, pitch=64):
    kernel, C = fx["kernel"], fx["C"]
    o, ot = run(ops, kernel, device_operands(fx, pitch), M, C, tag)
    assert_equal(f"{kernel} outt against out (randn)", ot, o.to(BF16), tag)
    a = assert_within(f"{kernel} out (randn)", o, fx["ref"], fx["bound"], tag)
    b = assert_within(f"{kernel} outt (randn)", ot, fx["ref"], fx["bound_t"], tag)
    return a, b


# ---------------------------------------------------------------------------------------------------------------- proj
@pytest.mark.parametrize("mu", T.MUS)
@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("M", T.PROJ_M)
def test_proj_exact(ops, M, C, mu):
    check_exact(ops, T.take_rows(T.proj_fixture(C, mu), M), M, f" M={M} C={C} mu={mu}")


@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("M", T.PROJ_M)
def test_proj_randn_per_element(ops, M, C):
    check_randn(ops, T.take_randn_rows(T.proj_randn(C), M), M, f" M={M} C={C}")


# ---------------------------------------------------------------------------------------------------------------- mlp
@pytest.mark.parametrize("mu", T.MUS)
@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("M", T.MLP_M)
def test_mlp_exact(ops, M, C, mu):
    check_exact(ops, T.take_rows(T.mlp_fixture(C, mu), M), M, f" M={M} C={C} mu={mu}")


@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("M", T.MLP_M)
def test_mlp_randn_per_element(ops, M, C):
    check_randn(ops, T.take_randn_rows(T.mlp_randn(C), M), M, f" M={M} C={C}")


@pytest.mark.parametrize("C", [64, 128])
def test_mlp_gelu_sweep_per_element(ops, C):
    # one hidden unit per channel, every multiple of 1/64 in [-6, 6): the same expression, tight where gelu_poly works
    fx = T.mlp_sweep(C)
    check_randn(ops, fx, T.SWEEP_M, f" gelu sweep C={C}")


# ---------------------------------------------------------------------------------------------------------------- linear_ln
LINLN = [(M, K) for K, Ms in T.LINLN_M.items() for M in Ms]


@pytest.mark.parametrize("mu", T.MUS)
@pytest.mark.parametrize("M,K", LINLN)
def test_linear_ln_exact(ops, M, K, mu):
    check_exact(ops, T.take_rows(T.linln_fixture(K, mu), M), M, f" M={M} K={K} mu={mu}")


@pytest.mark.parametrize("M,K", LINLN)
def test_linear_ln_randn_per_element(ops, M, K):
    check_randn(ops, T.take_randn_rows(T.linln_randn(K), M), M, f" M={M} K={K}")


# ---------------------------------------------------------------------------------------------------------------- patch_embed
EMBED = [(B, HW, C, mu) for B, HW in T.EMBED_SHAPES for C in (64, 96, 128) for mu in T.MUS if C != 96 or mu == 0]  # f32(1 / 96) is inexact


@pytest.mark.parametrize("pitch", T.EMBED_PITCH)
@pytest.mark.parametrize("B,HW,C,mu", EMBED)
def test_patch_embed_exact(ops, B, HW, C, mu, pitch):
    fx = T.embed_fixture(B, HW, C, mu)
    check_exact(ops, fx, fx["x"].shape[0], f" B={B} HW={HW} C={C} mu={mu} pitch={pitch}", pitch)


@pytest.mark.parametrize("pitch", T.EMBED_PITCH)
@pytest.mark.parametrize("C", [64, 96, 128])
@pytest.mark.parametrize("B,HW", T.EMBED_SHAPES)
def test_patch_embed_randn_per_element(ops, B, HW, C, pitch):
    fx = T.embed_randn(B, HW, C)
    check_randn(ops, fx, fx["x"].shape[0], f" B={B} HW={HW} C={C} pitch={pitch}", pitch)


# ---------------------------------------------------------------------------------------------------------------- refusals
def refused(ops, kernel, t, M, C, tag):
    out, outt = Guarded((M, C), F32), Guarded((M, C), BF16)
    with pytest.raises(NotImplementedError):
        launch(ops, kernel, t, out.t, outt.t)
    torch.cuda.synchronize()
    for name, g in (("out", out), ("outt", outt)):
        v = g.check(f"{kernel} {name}{tag}")
        assert bool(torch.isnan(v.float()).all()), f"{kernel} {name}{tag}: a refused call wrote {int((~torch.isnan(v.float())).sum())} elements"


def zeros_case(kernel, M, C, K):
    t = dict(x=torch.zeros(M, K, dtype=BF16).cuda(), sc=torch.zeros(M, C).cuda(), gamma=torch.ones(C).cuda(), beta=torch.zeros(C).cuda(),
             b=torch.zeros(C).cuda())
    if kernel == "mlp":
        t.update(W1=torch.zeros(4 * C, C, dtype=BF16).cuda(), b1=torch.zeros(4 * C).cuda(), W=torch.zeros(C, 4 * C, dtype=BF16).cuda())
    else:
        t.update(W=torch.zeros(C, K, dtype=BF16).cuda())
    return t


@pytest.mark.parametrize("kernel", ["mlp", "proj"])
def test_mlp_and_proj_refuse_c_256(ops, kernel):
    refused(ops, kernel, zeros_case(kernel, 8, 256, 256), 8, 256, " C=256")


@pytest.mark.parametrize("C,K", [(128, 128), (256, 96), (256, 144)])
def test_linear_ln_refuses_outside_its_envelope(ops, C, K):
    refused(ops, "linear_ln", zeros_case("linear_ln", 8, C, K), 8, C, f" C={C} K={K}")


def test_patch_embed_refuses_patch_2_and_c_256(ops):
    pix = torch.zeros(1, 3, 8, 8).cuda()
    for C, patch in ((64, 2), (256, 4)):
        M = (8 // patch) ** 2
        out, outt = Guarded((M, C), F32), Guarded((M, C), BF16)
        with pytest.raises(NotImplementedError):
            ops.swin_patch_embed_fused(pix, torch.zeros(C, 64, dtype=BF16).cuda(), torch.zeros(C).cuda(), torch.ones(C).cuda(), torch.zeros(C).cuda(),
                                       out.t, outt.t, patch=patch)
        torch.cuda.synchronize()
        for name, g in (("out", out), ("outt", outt)):
            assert bool(torch.isnan(g.check(f"patch_embed {name} C={C} patch={patch}").float()).all()), f"patch_embed {name}: a refused call wrote"
