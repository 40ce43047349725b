"""Frozen-tower window attention on the pre-arranged bias image (klab_swin_bias_image / klab_swin_qkv_attn_fused_img).

The image holds, per (window class, head), bias + shift mask + key padding in the order in which a lane of the score MFMA holds its
16 scores of a query tile; the kernel that reads it must give the very bits of the dense-table kernel klab_swin_qkv_attn_fused.
"""
import types

import pytest
import torch

from tests.helpers import rel_l2

pytestmark = pytest.mark.gpu

SHAPES = [(14, 64, 2, 0, 7), (14, 64, 2, 3, 7), (14, 128, 4, 3, 7), (7, 128, 4, 0, 7), (14, 256, 8, 3, 7), (14, 256, 8, 0, 7),
          (16, 64, 2, 4, 8), (8, 128, 4, 0, 8), (16, 256, 8, 4, 8)]  # (R, C, H, shift, w)


@pytest.fixture(scope="module")
def ops():
    from klab_multimodalmodel_amd import ops as K
    return K


def region(s, R, w, shift):
    return (s >= R - w).long() + (s >= R - shift).long()


def image_reference(bias, R, w, shift):
    """[classes, H, 4, 64, 16] from the dense bias [H, n, n]: class = 2 * (last window row) + (last window column)."""
    H, n = bias.shape[0], w * w
    lane, j = torch.arange(64), torch.arange(16)
    qt = torch.arange(4)
    q = (qt[:, None, None] * 16 + (lane[None, :, None] & 15)).expand(4, 64, 16)
    key = ((j[None, None, :] >> 2) * 16 + (lane[None, :, None] >> 4) * 4 + (j[None, None, :] & 3)).expand(4, 64, 16)
    qc, kc = q.clamp(max=n - 1), key.clamp(max=n - 1)
    out = []
    for cls in range(4 if shift > 0 else 1):
        val = bias[:, qc, kc].clone()  # [H, 4, 64, 16]
        if shift > 0:
            wy, wx = (R // w - 1) * (cls >> 1), (R // w - 1) * (cls & 1)  # any window that is not last has region 0 throughout

            def reg(slot):
                return region(wy * w + slot // w, R, w, shift) * 3 + region(wx * w + slot % w, R, w, shift)
            val = torch.where(reg(qc) != reg(kc), val + -200.0, val)
        val = torch.where(key < n, val, torch.full_like(val, float("-inf")))
        out.append(val)
    return torch.stack(out)


@pytest.mark.parametrize("R,w,shift,H", [(14, 7, 3, 2), (14, 7, 0, 2), (7, 7, 0, 4), (16, 8, 4, 8)])
def test_bias_image_matches_torch(ops, R, w, shift, H):
    n = w * w
    bias = 16 * torch.sigmoid(torch.randn(H, n, n, generator=torch.Generator().manual_seed(4)))
    ref = image_reference(bias, R, w, shift)
    if shift > 0 and R // w > 1:  # the rule the classes rest on: outside the last window row / column every region is 0
        s = torch.arange(R - w)
        assert int(region(s, R, w, shift).max()) == 0
    img = ops.swin_bias_image(bias.cuda(), R=R, w=w, shift=shift)
    assert tuple(img.shape) == (4 if shift > 0 else 1, H, 4, 64, 16)
    assert torch.equal(img.cpu(), ref)
    if n < 64:
        assert torch.isinf(ref).any()


_cache = {}


def fused_case(ops, R, Cc, Hh, shift, w, with_bias, B=3):
    """inputs of test_swin_qkv_attn_fused_matches_two_kernel_path; dense-table ctx, image ctx and the two-kernel ctx, computed once"""
    key = (R, Cc, Hh, shift, w, with_bias, B)
    if key in _cache:
        return _cache[key]
    n = w * w
    g = torch.Generator().manual_seed(9)
    M = B * R * R
    x = torch.randn(M, Cc, generator=g).to(torch.bfloat16).cuda()
    wq = (torch.randn(3 * Cc, Cc, generator=g) / Cc ** 0.5).to(torch.bfloat16).cuda()
    bq = torch.randn(3 * Cc, generator=g) * 0.2
    bq[Cc:2 * Cc] = 0
    bq = bq.cuda() if with_bias else None
    bias = torch.randn(Hh, n, n, generator=g).cuda()
    ls = torch.full((Hh,), 2.0).cuda()
    kw = dict(B=B, R=R, w=w, shift=shift, H=Hh, C=Cc)
    old = torch.zeros(M, Cc, device="cuda", dtype=torch.bfloat16)
    ops.swin_qkv_attn_fused(x, wq, bq, old, bias, ls, **kw)
    img = ops.swin_bias_image(bias, R=R, w=w, shift=shift)
    new = torch.zeros(M, Cc, device="cuda", dtype=torch.bfloat16)
    ops.swin_qkv_attn_fused_img(x, wq, bq, new, img, ls, **kw)  # NotImplementedError (UNSUPPORTED) on a listed shape fails the test
    qkv = torch.empty(M, 3 * Cc, device="cuda", dtype=torch.bfloat16)
    ops.gemm(x, wq, qkv, M=M, N=3 * Cc, K=Cc, bias=bq)
    two = torch.empty(M, Cc, device="cuda", dtype=torch.bfloat16)
    ops.swin_attn_fwd(qkv, two, bias, ls, None, **kw)
    _cache[key] = (old.cpu(), new.cpu(), two.cpu())
    return _cache[key]


@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("R,Cc,Hh,shift,w", SHAPES)
def test_image_kernel_bit_equals_dense_table_kernel(ops, R, Cc, Hh, shift, w, with_bias):
    old, new, _ = fused_case(ops, R, Cc, Hh, shift, w, with_bias)
    assert torch.isfinite(new.float()).all()
    assert torch.equal(old, new), (old.float() - new.float()).abs().max()


@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("R,Cc,Hh,shift,w", SHAPES)
def test_image_kernel_matches_two_kernel_path(ops, R, Cc, Hh, shift, w, with_bias):
    """pinned to the oracle-pinned form (klab_gemm + klab_swin_attn_fwd) directly, at the bound of the dense-table kernel's test"""
    _, new, two = fused_case(ops, R, Cc, Hh, shift, w, with_bias)
    assert rel_l2(new.float(), two.float()) < 1.5e-2


def test_engine_rebuilds_the_image_with_the_weight_version():
    """Frozen bf16 tower at the window-8 geometry of test_reference_default_window_geometry_matches_oracle (stages 1-3: C = 64 / 128 / 256
    on the image): after a change of a shifted block's position-bias MLP the loss is that of an engine bound afresh to the new weights."""
    from klab_multimodalmodel_amd.engine import SwinConfig, T5Config
    from klab_multimodalmodel_amd.models.model import MyModel
    sw = SwinConfig(image_size=256, embed_dim=32, depths=(2, 2, 2, 2), num_heads=(1, 2, 4, 8), window_size=8)
    t5 = T5Config(vocab_size=512, d_model=256, d_kv=32, num_heads=4, d_ff=512, num_layers=2)
    args = types.SimpleNamespace(result_dir="/tmp", language_model_name="-", image_model_name="-", image_model_train=False,
                                 transformer_model_name="-")
    g = torch.Generator().manual_seed(5)
    pix = torch.randn(2, 3, 256, 256, generator=g).cuda()
    src, tgt = torch.randint(2, 500, (2, 5), generator=g).cuda(), torch.randint(2, 500, (2, 9), generator=g).cuda()

    def loss_of(m):
        return m({"pixel_values": pix}, {"input_ids": src}, {"input_ids": tgt}).item()

    m = MyModel(args, _configs=(sw, t5, t5), _seed=39, dtype=torch.bfloat16).to("cuda")
    m.transformer.eval()
    with torch.no_grad():
        l1 = loss_of(m)
        assert loss_of(m) == l1
        sd = {k: v.detach().clone() for k, v in m.image_model.state_dict().items()}
        for name in ("encoder.layers.1.blocks.1", "encoder.layers.2.blocks.1", "encoder.layers.3.blocks.0"):
            sd[name + ".attention.self.continuous_position_bias_mlp.2.weight"] *= -3.0
        m.image_model.load_state_dict(sd)
        l2 = loss_of(m)
        assert l2 != l1
        sds = [{k: v.detach().cpu().clone() for k, v in t.state_dict().items()} for t in (m.image_model, m.language_model, m.transformer)]
        fresh = MyModel(args, _configs=(sw, t5, t5), _state_dicts=tuple(sds), dtype=torch.bfloat16).to("cuda")
        fresh.transformer.eval()
        assert loss_of(fresh) == l2
